#!/usr/bin/env python
"""The VGG16 backbone's pool kernel, its convolutions and its captured frame.  Same process, same device.

(a) pools   the four 2x2 / stride 2 max-pool calls of a 1000 x 600 frame (``ops.maxpool2x2s2_nhwc``: 600 x 1000 x 64 down to
            75 x 125 x 512).  ``--inner``
            back-to-back calls are captured into one hipGraph (kernel nodes only); the calls of a graph walk a ring of
            buffer sets so that consecutive calls do not touch the same bytes; a window is one replay between two device
            events.  Next to each call a ``torch`` device copy that moves the same number of bytes through a ring of the
            same footprint, timed in alternating windows: the streaming yardstick.  Bytes of a pool call: 4 * (the input
            floats inside the windows + the output floats) - 4/5 read, 1/5 written; the copy reads half and writes half.
            Rings whose footprint fits the 256 MiB Infinity Cache are marked: their rate is a cache rate.
(b) convs   the 13 convolutions of the head at that frame size and fc6 / fc7 at 300 RoIs, each through the call the net
            makes (``hip_modules.conv_forward``; fp32 unless the library's split-bf16 rule takes the layer): the plan of
            the library's model (its split-K count, read off the workspace), the workspace, the time per call and the
            achieved TFLOP/s of the direct-convolution count 2 * M * K * R * S * C.  For the record, the two layers with the
            largest workspaces are also timed with other split-K counts forced (``split_k=``), and fc6 through the
            split-bf16 kernel.
(c) frame   the captured VGG16 frame (``model/frame_graph.FrameRunner``: 1000 x 600, 300 proposals, 2 classes, filter
            included) with one and with four frames in flight, and the ResNet-101 frame of the same process beside it (its
            convolution plans from the committed table, VGG16's from the library's rule).

    python tools/vgg16_bench.py [--out profiles/vgg16.md]
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
POOL_CALLS = [(1, 600, 1000, 64), (1, 300, 500, 128), (1, 150, 250, 256), (1, 75, 125, 512)]
# (h, w, c, k) of the head's 13 convolutions on a 600 x 1000 blob (3x3 / pad 1; the first reads the image padded to 4)
CONV_CALLS = [(600, 1000, 4, 64), (600, 1000, 64, 64), (300, 500, 64, 128), (300, 500, 128, 128), (150, 250, 128, 256),
              (150, 250, 256, 256), (150, 250, 256, 256), (75, 125, 256, 512), (75, 125, 512, 512), (75, 125, 512, 512),
              (37, 62, 512, 512), (37, 62, 512, 512), (37, 62, 512, 512)]
FC_CALLS = [("fc6", 300, 25088, 4096), ("fc7", 300, 4096, 4096)]
TILES = ("256x128", "128x256", "128x128", "128x64", "64x128", "64x64", "128x128 dma2", "64x64 dma", "128x64 dma",
         "64x128 dma", "128x128 dma", "256x128 dma", "128x256 dma", "64x64 persistent")


def alternate(windows, reps, warmup):
    out = {k: [] for k in windows}
    for r in range(warmup + reps):
        for k, fn in windows.items():
            t = fn()
            if r >= warmup:
                out[k].append(t)
    return out


def plan_text(ws_bytes, out_floats):
    """Nothing is tuned and no plan is imported for these shapes, so a call runs the library's analytic model: an implicit
    GEMM whose split-K count shows in its workspace, one M x K slab of partial sums per split."""
    splits = ws_bytes // (4 * out_floats) if ws_bytes else 1
    return "implicit GEMM, %d split%s" % (splits, "" if splits == 1 else "s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--no-pools", action="store_true")
    ap.add_argument("--no-convs", action="store_true")
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--no-resnet", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.nets import hip_modules
    assert torch.cuda.is_available(), "vgg16_bench needs the MI355X"
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
        for c in (calls[0], calls[0]) + tuple(calls[1:2]):      # the second call of a layer may build a derived filter
            c()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for c in calls:
                c()
        return graph

    def stats(v):
        return float(np.median(v)), float(min(v))

    lines = ["# VGG16 backbone: the 2x2 max-pool, the convolutions and the captured frame (`tools/vgg16_bench.py`)", "",
             "Command: `python tools/vgg16_bench.py --out profiles/vgg16.md` (reps %d, warm-up %d, %d calls per call window, "
             "%d frames per frame window)." % (args.reps, args.warmup, args.inner, args.frames)]

    if not args.no_pools:
        lines += ["", "## (a) The four max-pool calls of a 1000 x 600 frame", "",
                  "Device-event interval of one hipGraph replay holding %d back-to-back calls, per call; median (minimum) of %d "
                  "windows, the kernel and the copy alternating.  The calls of a graph walk a ring of buffer sets (the "
                  "footprint column); a footprint of at most 256 MiB fits the Infinity Cache, and its rates are CACHE rates "
                  "(marked `cache`).  Bytes of a pool call: 4 * (input floats inside the windows + output floats), 4/5 read and "
                  "1/5 written; the copy moves the same number, half read and half written.  Share of peak: bytes over the time "
                  "at the 8.0 TB/s HBM peak (a float4 copy reaches 6.29 TB/s of it)."
                  % (args.inner, args.reps), "",
                  "| shape (n,h,w,c) | MB | ring footprint MB | us per call | GB/s | share of HBM peak | copy us | copy GB/s | kernel / copy rate |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for n, h, w, c in POOL_CALLS:
            ho, wo = h // 2, w // 2
            nbytes = 4 * (n * 2 * ho * 2 * wo * c + n * ho * wo * c)
            sets = int(min(args.inner, max(1, -(-RING_BYTES // nbytes))))
            xs = [torch.randn((n, h, w, c), device=dev, generator=g) for _ in range(sets)]
            ys = [torch.empty((n, ho, wo, c), device=dev) for _ in range(sets)]
            half = max(nbytes // 8, 1)
            src = [torch.rand(half, device=dev, generator=g) for _ in range(sets)]
            dst = [torch.empty(half, device=dev) for _ in range(sets)]
            order = [i % sets for i in range(args.inner)]
            pools = [(lambda x=x, y=y: ops.maxpool2x2s2_nhwc(x, out=y)) for x, y in zip(xs, ys)]
            copies = [(lambda s=s, d=d: d.copy_(s)) for s, d in zip(src, dst)]
            graphs = {"kernel": captured([pools[i] for i in order]), "copy": captured([copies[i] for i in order])}
            t = {k: stats(v) for k, v in alternate({k: timed_replay(v, args.inner) for k, v in graphs.items()}, args.reps,
                                                   args.warmup).items()}
            del graphs, xs, ys, src, dst, pools, copies
            torch.cuda.empty_cache()
            foot = sets * nbytes
            (tk, tkm), (tc, tcm) = t["kernel"], t["copy"]
            lines.append("| (%d,%d,%d,%d) | %.2f | %.0f%s | %.1f (%.1f) | %.0f | %.1f %% | %.1f (%.1f) | %.0f | %.2f |"
                         % (n, h, w, c, nbytes / 1e6, foot / 1e6, " `cache`" if foot <= INFINITY_CACHE else "", tk * 1e6,
                            tkm * 1e6, nbytes / tk / 1e9, 100 * nbytes / tk / HBM_PEAK, tc * 1e6, tcm * 1e6,
                            nbytes / tc / 1e9, tc / tk))

    if not args.no_convs:
        lib = _hip.load()
        hip_modules.set_net_mode('TEST')
        lines += ["", "## (b) The convolutions of a 1000 x 600 frame and fc6 / fc7 at 300 RoIs", "",
                  "Each layer through ``hip_modules.conv_forward`` with bias and ReLU, the call the net makes (cfg defaults: "
                  "CONV_BF16 off, CONV_SPLIT_BF16 on - `split-bf16 rule` says whether the library's rule takes the layer).  "
                  "Plan: the library's analytic model (nothing is tuned or imported for these shapes; the split-K count is read off the "
                  "workspace, one M x K slab per split; rows marked `forced` pass ``split_k=``).  %d back-to-back calls in one hipGraph "
                  "over a ring of activation sets, per call; median (minimum) of %d windows.  TFLOP/s: 2 * M * K * R * S * C "
                  "over the time." % (min(args.inner, 10), args.reps), "",
                  "| layer | M x C -> K | GFLOP | plan | split-bf16 rule | workspace MB | us per call | TFLOP/s |", "|---|---|---|---|---|---|---|---|"]
        inner = min(args.inner, 10)

        class Holder(object):
            pass

        def time_layer(name, n, h, w, c, k, r, pad, call=None, split_k=0):
            wt = (torch.randn((k, r, r, c), device=dev, generator=g) * float(np.sqrt(2.0 / (r * r * c)))).contiguous()
            bias = torch.rand((k,), device=dev, generator=g) * 0.2 - 0.1
            x_bytes = 4 * n * h * w * (c + k)
            sets = int(min(inner, max(1, -(-RING_BYTES // x_bytes))))
            xs = [torch.randn((n, h, w, c), device=dev, generator=g) for _ in range(sets)]
            holder = Holder()
            if split_k:
                call = lambda x: ops.conv2d_nhwc(x, wt, None, bias, None, stride=1, pad=pad, relu=True, split_k=split_k)
            elif call is None:
                call = lambda x: hip_modules.conv_forward(x, wt, None, bias, None, holder, stride=1, pad=pad, relu=True,
                                                          winograd_of=holder if r == 3 else None)
            else:
                call = call(wt, bias)
            calls = [(lambda x=x: call(x)) for x in xs]
            graph = captured([calls[i % sets] for i in range(inner)])
            med, low = stats(alternate({"k": timed_replay(graph, inner)}, args.reps, args.warmup)["k"])
            flops = 2.0 * n * h * w * k * r * r * c
            ws = lib.frcnn_conv2d_fwd_ws_bytes(n, h, w, c, k, r, r, 1, pad, split_k)
            rule = bool(lib.frcnn_conv2d_split_bf16_wanted(n, h, w, c, k, r, r, 1, pad)) if c % 32 == 0 else False
            plan = plan_text(ws, n * h * w * k) + (" forced" if split_k else "")
            lines.append("| %s | %d x %d -> %d | %.1f | %s | %s | %.1f | %.1f (%.1f) | %.1f |"
                         % (name, n * h * w, r * r * c, k, flops / 1e9, plan, "yes" if rule else "no", ws / 1e6, med * 1e6,
                            low * 1e6, flops / med / 1e12))
            del graph, calls, xs, wt
            torch.cuda.empty_cache()

        with torch.no_grad():
            for i, (h, w, c, k) in enumerate(CONV_CALLS):
                time_layer("features.%d %dx%d" % ((0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)[i], h, w), 1, h, w, c, k, 3, 1)
            for name, m, c, k in FC_CALLS:
                time_layer(name, m, 1, 1, c, k, 1, 0)

            def forced_split(wt, bias):
                packed = ops.conv2d_pack_bf16x3(wt)
                return lambda x: ops.conv2d_nhwc_bf16x3(x, packed, None, bias, None, relu=True)
            name, m, c, k = FC_CALLS[0]
            time_layer(name + " split-bf16 forced", m, 1, 1, c, k, 1, 0, call=forced_split)
            lines[-1] = lines[-1].replace("| no |", "| forced |").replace("| yes |", "| forced |").replace("implicit GEMM, 8 splits", "split-bf16")
            for sk in (1, 2, 3):
                time_layer("features.19 75x125", 1, 75, 125, 512, 512, 3, 1, split_k=sk)
            for sk in (2, 4, 16):
                time_layer(name, m, 1, 1, c, k, 1, 0, split_k=sk)
        hip_modules.set_net_mode(None)

    if not args.no_frame:
        from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
        from faster_rcnn_pytorch_multimodal_amd.model.streams import concurrent_streams
        from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
        from faster_rcnn_pytorch_multimodal_amd.nets.vgg16 import vgg16
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
        torch.manual_seed(7)
        nets = {"VGG16": vgg16()}
        if not args.no_resnet:
            nets["ResNet-101"] = imagenet(num_layers=101)
        runners, rois, resident = {}, {}, {}
        for name, net in nets.items():
            net.create_architecture(2, tag="default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
            if not name.startswith("VGG"):       # VGG16 keeps its constructor's initialisation (torch.manual_seed(7))
                net.load_state_dict(seeded_state_dict(net, 7, bn_mode="tame"), strict=True)
            net.eval()
            net._device = dev
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            net.to(dev)
            runners[name] = []
            for s in streams:
                with torch.cuda.stream(s):
                    runners[name].append(FrameRunner(net, h, w, 3, info, thresh=0.05, max_dets=100, autotune=False))
                torch.cuda.synchronize()
            runners[name][0].run(blob)
            torch.cuda.synchronize()
            rois[name] = int(runners[name][0].predictions["rois_count"].item())
            params = sum(p.numel() * 4 for p in net.parameters()) + sum(b.numel() * b.element_size() for b in net.buffers())
            resident[name] = (params, torch.cuda.memory_allocated() - before)

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
        lines += ["", "## (c) The captured frame, 1000 x 600, 2 classes", "",
                  "One captured frame per stream (filter included); host clock around %d replays that end in a device "
                  "synchronise, per frame; median (minimum) of %d windows, the nets alternating.  ResNet-101: seeded weights, the "
                  "convolution plans of the committed table; VGG16: the constructor's initialisation, the library's default rule, "
                  "nothing tuned." % (args.frames, args.reps), "",
                  "| net | proposals | frames in flight | ms per frame | frames/s |", "|---|---|---|---|---|"]
        for lanes in (1, 4):
            t = alternate({name: frame_window(rs, lanes) for name, rs in runners.items()}, args.reps, args.warmup)
            for name, v in t.items():
                med = float(np.median(v))
                lines.append("| %s | %d | %d | %.3f (%.3f) | %.1f |" % (name, rois[name], lanes, med * 1e3, min(v) * 1e3, 1 / med))
        lines += ["", "Device memory: parameters and buffers, and everything allocated once four captured frames exist "
                  "(parameters, derived weights - KRSC filters, fc6's permuted copy - and the graphs' pools): "
                  + "; ".join("%s %.0f MB / %.0f MB" % (k, v[0] / 1e6, v[1] / 1e6) for k, v in resident.items()) + "."]
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
