#!/usr/bin/env python
"""Training the MobileNet-v1 detector: the three backward streaming kernels and the training step.  Same process, same device.

(a) kernels  ``ops.depthwise_conv3x3_bwd_data``, ``ops.depthwise_conv3x3_bwd_weight`` and ``ops.act_bwd_cap`` on the shapes
             of a 1000 x 600 frame with cfg.MOBILENET.FIXED_LAYERS = 5 and 256 sampled RoIs: the depthwise layers of
             Conv2d_5 .. Conv2d_11 on the map and of Conv2d_12 / Conv2d_13 on the pooled RoIs (both stride 1 in this body's
             table, lib/nets/mobilenet_v1.py:46-48), and the pointwise outputs behind them.  Method of
             tools/mobilenet_bench.py: ``--inner`` back-to-back calls captured into one hipGraph walking a ring of buffer
             sets, a window is one replay between two device events, and next to each call a ``torch`` device copy that
             moves the same number of bytes, timed in alternating windows.  Bytes (what the definition has to move):
             bwd_data 4 * (2 * out + in + 13 * C), bwd_weight 4 * (in + 2 * out + 13 * C) - its workgroup partials, written
             and read once more, are NOT counted and are listed beside it -, act_bwd_cap 4 * (3 * count + k).
(b) steps    one 1000 x 600 frame with three boxes: the eager step, the captured step (``enable_train_graphs``) and
             ``TrainPipeline`` with ``--inflight`` frames in flight, for MobileNet-v1 (cfg.TRAIN.MOBILENET_EN) and, in the same
             process, the ResNet-101 detector without FPN.  Host clock around windows that end in a device synchronise
             (tools/bench_configs.py's windows: a weight update every 16 frames).

    python tools/mobilenet_train_bench.py [--out profiles/mobilenet_train.md]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12
INFINITY_CACHE = 256 << 20
RING_BYTES = 640 << 20
# (layers, n, h, w, c, stride, the layer's input takes a gradient) - the input of Conv2d_5 comes from a frozen child
DW_LAYERS = [("Conv2d_5", 1, 75, 125, 256, 1, False), ("Conv2d_6", 1, 75, 125, 256, 2, True),
             ("Conv2d_7..11", 1, 38, 63, 512, 1, True), ("Conv2d_12", 256, 7, 7, 512, 1, True),
             ("Conv2d_13", 256, 7, 7, 1024, 1, True)]
# pointwise outputs (rows, k)
ACT_LAYERS = [("Conv2d_5", 75 * 125, 256), ("Conv2d_6..11", 38 * 63, 512), ("Conv2d_12..13", 256 * 7 * 7, 1024)]


def alternate(windows, reps, warmup):
    out = {k: [] for k in windows}
    for r in range(warmup + reps):
        for k, fn in windows.items():
            t = fn()
            if r >= warmup:
                out[k].append(t)
    return out


def spread(v):
    return "%.1f (%.1f - %.1f)" % (float(np.median(v)) * 1e6, min(v) * 1e6, max(v) * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-resnet", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    assert torch.cuda.is_available(), "mobilenet_train_bench needs the MI355X"
    dev = "cuda:0"
    lib = _hip.load()
    g = torch.Generator(device=dev).manual_seed(5)
    rand = lambda *shape: torch.rand(shape, device=dev, generator=g)

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

    def measure(make_call, nbytes):
        """make_call() builds one buffer set and returns the call on it.  Returns {kernel / copy: window times}, sets."""
        sets = int(min(args.inner, max(1, -(-RING_BYTES // nbytes))))
        calls = [make_call() for _ in range(sets)]
        half = max(nbytes // 8, 1)
        src = [rand(half) for _ in range(sets)]
        dst = [torch.empty(half, device=dev) for _ in range(sets)]
        copies = [(lambda s=s, d=d: d.copy_(s)) for s, d in zip(src, dst)]
        order = [i % sets for i in range(args.inner)]
        graphs = {"kernel": captured([calls[i] for i in order]), "copy": captured([copies[i] for i in order])}
        t = alternate({k: timed_replay(v, args.inner) for k, v in graphs.items()}, args.reps, args.warmup)
        del calls, graphs, src, dst
        torch.cuda.empty_cache()
        return t, sets

    lines = ["# Training MobileNet-v1: the backward streaming kernels and the training step (`tools/mobilenet_train_bench.py`)", "",
             "Command: `python tools/mobilenet_train_bench.py --out profiles/mobilenet_train.md` (reps %d, warm-up %d, %d calls "
             "per kernel window, %d steps per step window)." % (args.reps, args.warmup, args.inner, args.steps), "",
             "## (a) The backward kernels on the shapes of a 1000 x 600 frame, FIXED_LAYERS = 5, 256 sampled RoIs", "",
             "Device-event interval of one hipGraph replay holding %d back-to-back calls, per call; median (minimum - maximum) "
             "of %d windows, kernel and copy alternating.  The calls of a graph walk a ring of buffer sets; a ring of at most "
             "256 MiB fits the Infinity Cache and its rates are CACHE rates (marked `cache`).  The copy moves the same number "
             "of bytes (half read, half written).  `bwd_weight` is its two launches together; the partials column is what "
             "its workgroups write and its second launch reads on top of the counted bytes." % (args.inner, args.reps), "",
             "| kernel | layers | shape (n,h,w,c) / stride | MB | ring MB | us per call | TB/s | share of the 8.0 TB/s HBM peak | "
             "copy us | copy TB/s | kernel / copy rate | partials MB |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ratios = {}

    def row(kind, layers, shape, nbytes, t, sets, extra=""):
        tk, tc = float(np.median(t["kernel"])), float(np.median(t["copy"]))
        foot = sets * nbytes
        ratios.setdefault(kind, []).append((layers, tc / tk, nbytes))
        lines.append("| %s | %s | %s | %.2f | %.0f%s | %s | %.2f | %.1f %% | %s | %.2f | %.2f | %s |"
                     % (kind, layers, shape, nbytes / 1e6, foot / 1e6, " `cache`" if foot <= INFINITY_CACHE else "",
                        spread(t["kernel"]), nbytes / tk / 1e12, 100 * nbytes / tk / HBM_PEAK, spread(t["copy"]),
                        nbytes / tc / 1e12, tc / tk, extra))

    for layers, n, h, w, c, stride, need_dx in DW_LAYERS:
        oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
        n_in, n_out = n * h * w * c, n * oh * ow * c
        shape = "(%d,%d,%d,%d) / %d" % (n, h, w, c, stride)

        def operands():
            x = rand(n, h, w, c) * 8 - 1
            dy = rand(n, oh, ow, c) - 0.5
            y = (rand(n, oh, ow, c) * 8 - 1).clamp_(0, 6)
            return x, dy, y, rand(3, 3, c) - 0.5, rand(c) + 0.5

        if need_dx:
            def make_data():
                x, dy, y, wt, sc = operands()
                out = torch.empty_like(x)
                return lambda: ops.depthwise_conv3x3_bwd_data(dy, y, wt, (n, h, w, c), sc, stride=stride, relu=True, out_cap=6.0,
                                                              out=out)
            nbytes = 4 * (2 * n_out + n_in + 13 * c)
            t, sets = measure(make_data, nbytes)
            row("bwd_data", layers, shape, nbytes, t, sets, "-")

        def make_weight():
            x, dy, y, wt, sc = operands()
            out = torch.zeros((c, 1, 3, 3), device=dev)
            return lambda: ops.depthwise_conv3x3_bwd_weight(x, dy, y, sc, stride=stride, relu=True, in_cap=6.0, out_cap=6.0,
                                                            out=out, accumulate=True)
        nbytes = 4 * (n_in + 2 * n_out + 13 * c)
        t, sets = measure(make_weight, nbytes)
        row("bwd_weight", layers, shape, nbytes, t, sets, "%.2f" % (2 * lib.frcnn_dwconv3x3_bwd_weight_ws_bytes(n, h, w, c, stride) / 1e6))

    for layers, rows_, k in ACT_LAYERS:
        def make_act():
            dy, y, sc = rand(rows_, k) - 0.5, (rand(rows_, k) * 8 - 1).clamp_(0, 6), rand(k) + 0.5
            out = torch.empty_like(dy)
            return lambda: ops.act_bwd_cap(dy, y, sc, relu=True, cap=6.0, out=out)
        nbytes = 4 * (3 * rows_ * k + k)
        t, sets = measure(make_act, nbytes)
        row("act_bwd_cap", layers, "(%d,%d)" % (rows_, k), nbytes, t, sets, "-")
    lines += ["", "Kernel / copy rate per kernel, smallest to largest: " + "; ".join(
        "%s %s" % (kind, ", ".join("%.2f" % r for _, r, _ in sorted(v, key=lambda e: e[1]))) for kind, v in ratios.items())
        + ".  The forward kernel's yardstick on its large shapes: 0.44 - 0.56 (profiles/mobilenet.md)."]

    if not args.no_steps:
        import bench_configs as B
        from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
        from faster_rcnn_pytorch_multimodal_amd.nets.mobilenet_v1 import mobilenetv1
        from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
        h, w = 600, 1000
        rng = np.random.default_rng(3)
        blobs = {"data": (rng.standard_normal((1, h, w, 3)) * 50).astype(np.float32),
                 "info": np.array([0, w, 0, h, 0, 0, 1.0], np.float32),
                 "gt_boxes": np.array([[100, 80, 420, 380, 1], [520, 150, 900, 560, 1], [300, 300, 620, 590, 1]], np.float32),
                 "gt_boxes_dc": np.zeros((0, 4), np.float32)}
        lines += ["", "## (b) The training step, 1000 x 600, 2 classes, seeded weights, 3 boxes, 256 sampled RoIs", "",
                  "Host clock around %d steps that end in a device synchronise (a weight update every 16 frames), per step; "
                  "median of 3 windows after 8 untimed steps (tools/bench_configs.py's windows).  MobileNet-v1: "
                  "cfg.MOBILENET.FIXED_LAYERS = 5, its convolution plans tuned by the captured step's warm-up; ResNet-101 "
                  "without FPN: cfg.RESNET.FIXED_BLOCKS = 1." % args.steps, "",
                  "| net | mode | ms per step | steps/s |", "|---|---|---|---|"]
        for name in ["MobileNet-v1"] + ([] if args.no_resnet else ["ResNet-101"]):
            C.reset_cfg()
            C.cfg.NET_TYPE = "image"
            C.cfg.TRAIN.MOBILENET_EN = True
            torch.manual_seed(1)

            def build():
                net = mobilenetv1() if name.startswith("Mobile") else imagenet(num_layers=101)
                net.create_architecture(2, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
                sd = seeded_state_dict(net, 7, bn_mode="tame")
                if name.startswith("Mobile"):
                    body = seeded_state_dict(net, 7, bn_mode="tame", all_backbone=True)
                    sd.update({k: v for k, v in body.items() if k.startswith("mobilenet.")})
                net.load_state_dict(sd, strict=True)
                net._device = dev
                net.to(dev)
                net.train()
                return net, torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)
            for mode in ("eager", "captured", "pipeline x%d" % args.inflight):
                net, opt = build()
                if mode == "eager":
                    _, dt = B._timed_train_windows(net, blobs, opt, args.steps)
                elif mode == "captured":
                    net.enable_train_graphs(True)
                    _, dt = B._timed_train_windows(net, blobs, opt, args.steps)
                else:
                    _, dt = B._timed_pipeline_windows(net, blobs, opt, args.steps, args.inflight)
                lines.append("| %s | %s | %.2f | %.1f |" % (name, mode, 1e3 * dt / args.steps, args.steps / dt))
                print(lines[-1], flush=True)
                del net, opt
                torch.cuda.empty_cache()
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
