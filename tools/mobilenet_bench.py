#!/usr/bin/env python
"""The MobileNet-v1 backbone's streaming kernels and its captured frame.  Same process, same device.

(a) calls   the 13 depthwise 3x3 calls and the 2 ``clamp_max_`` calls of a 1000 x 600 frame with 300 RoIs (the 15 calls of
            the frame that are no GEMM): 300 x 500 x 32 down to 38 x 63 x 512 on the map, then 300 x 7 x 7 x 512 and
            300 x 7 x 7 x 1024 on the pooled RoIs.  ``--inner`` back-to-back calls are captured into one hipGraph (kernel
            nodes only); the calls of a graph walk a ring of buffer sets so that consecutive calls do not touch the same
            bytes; a window is one replay between two device events.  Next to each call a ``torch`` device copy that
            moves the same number of bytes (half read, half written) through a ring of the same footprint, timed in
            alternating windows: the streaming yardstick.  Bytes of a depthwise call: 4 * (in + out + 11 * C).  Rings
            whose footprint fits the 256 MiB Infinity Cache are marked: their rate is a cache rate, not an HBM rate.
(b) frame   the captured MobileNet frame (``model/frame_graph.FrameRunner``: 1000 x 600, 300 proposals, 2 classes, seeded
            weights, filter included) with one and with four frames in flight, and the ResNet-101 frame of the same
            process beside it (its convolution plans from the committed table, MobileNet's from the library's rule).

    python tools/mobilenet_bench.py [--out profiles/mobilenet.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12            # HBM3E spec peak; a float4 copy measures 6.29 TB/s of it
INFINITY_CACHE = 256 << 20
RING_BYTES = 640 << 20       # a ring grows towards this footprint (2.5 x the Infinity Cache), up to --inner sets
# (n, h, w, c, stride) of the depthwise calls, in frame order; the head's map sizes are those of a 600 x 1000 blob
DW_CALLS = ([(1, 300, 500, 32, 1), (1, 300, 500, 64, 2), (1, 150, 250, 128, 1), (1, 150, 250, 128, 2), (1, 75, 125, 256, 1),
             (1, 75, 125, 256, 2)] + [(1, 38, 63, 512, 1)] * 5 + [(300, 7, 7, 512, 1), (300, 7, 7, 1024, 1)])
CLAMP_CALLS = [(1, 38, 63, 512), (300, 7, 7, 1024)]       # net_conv and the tail's output


def alternate(windows, reps, warmup):
    out = {k: [] for k in windows}
    for r in range(warmup + reps):
        for k, fn in windows.items():
            t = fn()
            if r >= warmup:
                out[k].append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--no-resnet", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    assert torch.cuda.is_available(), "mobilenet_bench needs the MI355X"
    dev = "cuda:0"
    C.reset_cfg()
    cfg = C.cfg
    cfg.NET_TYPE = "image"
    g = torch.Generator(device=dev).manual_seed(5)

    def timed_replay(graph, units):
        def window():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3 / units
        return window

    def captured(calls):
        for c in calls[:2]:
            c()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for c in calls:
                c()
        return graph

    def measure(kernel_calls, nbytes, sets):
        """kernel_calls: ``sets`` callables (one per buffer set).  Returns (kernel s, copy s) medians and minima."""
        half = max(nbytes // 8, 1)                       # floats per side of a copy that moves nbytes
        src = [torch.rand(half, device=dev, generator=g) for _ in range(sets)]
        dst = [torch.empty(half, device=dev) for _ in range(sets)]
        copies = [(lambda s=s, d=d: d.copy_(s)) for s, d in zip(src, dst)]
        order = [i % sets for i in range(args.inner)]
        graphs = {"kernel": captured([kernel_calls[i] for i in order]), "copy": captured([copies[i] for i in order])}
        t = alternate({k: timed_replay(v, args.inner) for k, v in graphs.items()}, args.reps, args.warmup)
        return {k: (float(np.median(v)), float(min(v))) for k, v in t.items()}

    lines = ["# MobileNet-v1 backbone: the streaming kernels and the captured frame (`tools/mobilenet_bench.py`)", "",
             "Command: `python tools/mobilenet_bench.py --out profiles/mobilenet.md` (reps %d, warm-up %d, %d calls per call "
             "window, %d frames per frame window)." % (args.reps, args.warmup, args.inner, args.frames), "",
             "## (a) The 15 streaming calls of a 1000 x 600 frame with 300 RoIs", "",
             "Device-event interval of one hipGraph replay holding %d back-to-back calls, per call; median (minimum) of %d "
             "windows, kernel and copy alternating.  The calls of a graph walk a ring of buffer sets (the footprint column); "
             "a footprint of at most 256 MiB fits the Infinity Cache, and its rates are CACHE rates (marked `cache`).  Bytes "
             "of a depthwise call: 4 * (in + out + 11 * C); the copy moves the same number (half read, half written).  "
             "Share of peak: bytes over the time at the 8.0 TB/s HBM peak (a float4 copy reaches 6.29 TB/s of it)."
             % (args.inner, args.reps), "",
             "| call | shape (n,h,w,c) / stride | MB | ring footprint MB | us per call | GB/s | share of HBM peak | copy us | copy GB/s | kernel / copy rate |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    slow = []
    rows = [("depthwise",) + s for s in DW_CALLS] + [("clamp_max_",) + s + (0,) for s in CLAMP_CALLS]
    for kind, n, h, w, c, stride in rows:
        if kind == "depthwise":
            oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
            nbytes = 4 * (n * h * w * c + n * oh * ow * c + 11 * c)
        else:
            nbytes = 8 * n * h * w * c
        sets = int(min(args.inner, max(1, -(-RING_BYTES // nbytes))))
        calls = []
        for _ in range(sets):
            x = torch.rand((n, h, w, c), device=dev, generator=g) * 8 - 1
            if kind == "depthwise":
                wt = torch.rand((3, 3, c), device=dev, generator=g) - 0.5
                sc, sh = torch.rand((c,), device=dev, generator=g) + 0.5, torch.rand((c,), device=dev, generator=g)
                y = torch.empty((n, oh, ow, c), device=dev)
                calls.append(lambda x=x, wt=wt, sc=sc, sh=sh, y=y: ops.depthwise_conv3x3_nhwc(
                    x, wt, sc, sh, stride=stride, relu=True, in_cap=6.0, out_cap=6.0, out=y))
            else:
                calls.append(lambda x=x: ops.clamp_max_(x, 6.0))
        res = measure(calls, nbytes, sets)
        del calls
        torch.cuda.empty_cache()
        (tk, tk_min), (tc, tc_min) = res["kernel"], res["copy"]
        foot = sets * nbytes
        cache = foot <= INFINITY_CACHE
        lines.append("| %s | (%d,%d,%d,%d) / %s | %.2f | %.0f%s | %.1f (%.1f) | %.0f | %.1f %% | %.1f (%.1f) | %.0f | %.2f |"
                     % (kind, n, h, w, c, stride or "-", nbytes / 1e6, foot / 1e6, " `cache`" if cache else "", tk * 1e6,
                        tk_min * 1e6, nbytes / tk / 1e9, 100 * nbytes / tk / HBM_PEAK, tc * 1e6, tc_min * 1e6,
                        nbytes / tc / 1e9, tc / tk))
        if kind == "depthwise" and nbytes > 16e6 and tc / tk < 0.5:
            slow.append((n, h, w, c, stride, tc / tk))
    lines += ["", "Depthwise shapes above 16 MB that run below half of their copy yardstick: %s."
              % (", ".join("(%d,%d,%d,%d)/%d at %.2f" % s for s in slow) if slow else "none")]

    if not args.no_frame:
        from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
        from faster_rcnn_pytorch_multimodal_amd.model.streams import concurrent_streams
        from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
        from faster_rcnn_pytorch_multimodal_amd.nets.mobilenet_v1 import mobilenetv1
        from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
        h, w = 600, 1000
        info = np.array([0, w, 0, h, 0, 0, 1.0], np.float32)
        rng = np.random.default_rng(3)
        blob = torch.from_numpy((rng.standard_normal((1, h, w, 3)) * 50).astype(np.float32)).to(dev)
        streams, _ = concurrent_streams(4, torch.device(dev))
        plans = os.path.join(ROOT, "profiles", "r05_plans.json")
        if os.path.exists(plans):
            with open(plans) as f:
                ops.import_conv_plans(json.load(f))
        nets = {"MobileNet-v1": mobilenetv1()}
        if not args.no_resnet:
            nets["ResNet-101"] = imagenet(num_layers=101)
        runners, rois = {}, {}
        for name, net in nets.items():
            net.create_architecture(2, tag="default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
            sd = seeded_state_dict(net, 7, bn_mode="tame")
            if name.startswith("Mobile"):      # the body's convolutions get the backbone rule, like the resnet.* ones
                body = seeded_state_dict(net, 7, bn_mode="tame", all_backbone=True)
                sd.update({k: v for k, v in body.items() if k.startswith("mobilenet.")})
            net.load_state_dict(sd, strict=True)
            net.eval()
            net._device = dev
            net.to(dev)
            runners[name] = []
            for s in streams:
                with torch.cuda.stream(s):
                    runners[name].append(FrameRunner(net, h, w, 3, info, thresh=0.05, max_dets=100, autotune=False))
                torch.cuda.synchronize()
            runners[name][0].run(blob)
            torch.cuda.synchronize()
            rois[name] = int(runners[name][0].predictions["rois_count"].item())

        def frame_window(rs, lanes):
            def window():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.frames):
                    with torch.cuda.stream(streams[i % lanes]):
                        rs[i % lanes].run(blob)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.frames
            return window
        lines += ["", "## (b) The captured frame, 1000 x 600, 2 classes, seeded weights", "",
                  "One captured frame per stream (filter included); host clock around %d replays that end in a device "
                  "synchronise, per frame; median (minimum) of %d windows, the nets alternating.  ResNet-101: the convolution "
                  "plans of the committed table; MobileNet-v1: the library's default rule, nothing tuned."
                  % (args.frames, args.reps), "",
                  "| net | proposals | frames in flight | ms per frame | frames/s |", "|---|---|---|---|---|"]
        for lanes in (1, 4):
            t = alternate({name: frame_window(rs, lanes) for name, rs in runners.items()}, args.reps, args.warmup)
            for name, v in t.items():
                med = float(np.median(v))
                lines.append("| %s | %d | %d | %.3f (%.3f) | %.1f |" % (name, rois[name], lanes, med * 1e3, min(v) * 1e3, 1 / med))
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
