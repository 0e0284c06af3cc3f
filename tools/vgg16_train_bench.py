#!/usr/bin/env python
"""Training the VGG16 detector: the 2x2 max-pool gradient kernel, fc6's two gradient routes and the training step.  Same
process, same device.

(a) kernel   ``ops.maxpool2x2s2_bwd`` plain and with the ReLU mask (``relu=True``) at the two pools a training step
             differentiates on a 1000 x 600 frame - pool 16 on (1,150,250,256) and pool 23 on (1,75,125,512) - and the
             unfused pair ``maxpool2x2s2_bwd`` + ``act_bwd`` the fused form replaces.  Method of tools/vgg16_bench.py:
             ``--inner`` back-to-back calls captured into one hipGraph walking a ring of buffer sets, a window is one replay
             between two device events, and next to each call a ``torch`` device copy that moves the same number of bytes,
             timed in alternating windows.  Bytes of one call: 4 * (x + dy + dx) = 4 * (2 * in + out); of the pair:
             4 * (5 * in + out) (dx written, then dx and x read and the result written).
(b) fc6      relu(fc6) -> relu(fc7) forward and backward on 256 pooled RoIs through both routes of fc6's 411 MB filter
             gradient - the NCHW flattening with plain ``linear_train`` (``vgg16.FC6_NCHW_FLATTEN``) and the NHWC flattening
             against the permuted filter (``_PermutedLinearFn``) - under the eager schedule (gradients go back to autograd)
             and under the accumulating schedule of a captured step (in line, into existing ``param.grad``).  Device events
             around one forward + backward, the four forms alternating; peak device memory above the resident set.
(c) steps    one 1000 x 600 frame with three boxes: the eager step, the captured step (``enable_train_graphs``) and
             ``TrainPipeline`` with ``--inflight`` frames in flight, for VGG16 (cfg.TRAIN.VGG16_EN) and, in the same process,
             the ResNet-101 detector without FPN; device memory of the VGG16 forms.

    python tools/vgg16_train_bench.py [--out profiles/vgg16_train.md]
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
POOL_CALLS = [("pool 16", 1, 150, 250, 256), ("pool 23", 1, 75, 125, 512)]
ROIS = 256


def alternate(windows, reps, warmup):
    out = {k: [] for k in windows}
    for r in range(warmup + reps):
        for k, fn in windows.items():
            t = fn()
            if r >= warmup:
                out[k].append(t)
    return out


def spread(v, unit=1e6):
    return "%.1f (%.1f - %.1f)" % (float(np.median(v)) * unit, min(v) * unit, max(v) * unit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-fc6", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-resnet", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.nets import autograd_ops, hip_modules, vgg16 as V
    assert torch.cuda.is_available(), "vgg16_train_bench needs the MI355X"
    dev = "cuda:0"
    _hip.load()
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

    lines = ["# Training VGG16: the 2x2 max-pool gradient, fc6's gradient routes and the training step (`tools/vgg16_train_bench.py`)", "",
             "Command: `python tools/vgg16_train_bench.py --out profiles/vgg16_train.md` (reps %d, warm-up %d, %d calls per kernel "
             "window, %d steps per step window)." % (args.reps, args.warmup, args.inner, args.steps)]

    if not args.no_kernel:
        lines += ["", "## (a) `frcnn_maxpool2x2s2_bwd` at the two pools a 1000 x 600 training step differentiates", "",
                  "Device-event interval of one hipGraph replay holding %d back-to-back calls, per call; median (minimum - maximum) "
                  "of %d windows, kernel and copy alternating.  The calls of a graph walk a ring of buffer sets; a ring of at most "
                  "256 MiB fits the Infinity Cache and its rates are CACHE rates (marked `cache`).  The copy moves the same number "
                  "of bytes (half read, half written).  x is a ReLU output (half zeros).  `pair` is `maxpool2x2s2_bwd` followed by "
                  "`act_bwd` on the full-size gradient - what `relu=True` replaces; its copy moves the pair's bytes."
                  % (args.inner, args.reps), "",
                  "| form | pool | x (n,h,w,c) | MB | ring MB | us per call | TB/s | share of the 8.0 TB/s HBM peak | copy us | copy TB/s | "
                  "kernel / copy rate |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        fused_us = {}
        for pool, n, h, w, c in POOL_CALLS:
            n_in, n_out = n * h * w * c, n * (h // 2) * (w // 2) * c

            def operands():
                return (rand(n, h, w, c) - 0.5).relu_(), rand(n, h // 2, w // 2, c) - 0.5

            def make(form):
                def make_call():
                    x, dy = operands()
                    out = torch.empty_like(x)
                    if form == "pair":
                        return lambda: ops.act_bwd(ops.maxpool2x2s2_bwd(x, dy, out=out), x, None, relu=True)
                    return lambda: ops.maxpool2x2s2_bwd(x, dy, relu=(form == "relu"), out=out)
                return make_call
            for form in ("plain", "relu", "pair"):
                nbytes = 4 * ((5 if form == "pair" else 2) * n_in + n_out)
                t, sets = measure(make(form), nbytes)
                tk, tc = float(np.median(t["kernel"])), float(np.median(t["copy"]))
                fused_us[(pool, form)] = tk
                foot = sets * nbytes
                lines.append("| %s | %s | (%d,%d,%d,%d) | %.2f | %.0f%s | %s | %.2f | %.1f %% | %s | %.2f | %.2f |"
                             % (form, pool, n, h, w, c, nbytes / 1e6, foot / 1e6, " `cache`" if foot <= INFINITY_CACHE else "",
                                spread(t["kernel"]), nbytes / tk / 1e12, 100 * nbytes / tk / HBM_PEAK, spread(t["copy"]),
                                nbytes / tc / 1e12, tc / tk))
                print(lines[-1], flush=True)
        lines += ["", "Fused against the pair: " + "; ".join(
            "%s %.1f us against %.1f us (%.2fx)" % (pool, fused_us[(pool, "relu")] * 1e6, fused_us[(pool, "pair")] * 1e6,
                                                   fused_us[(pool, "pair")] / fused_us[(pool, "relu")]) for pool, *_ in POOL_CALLS) + "."]

    C.reset_cfg()
    C.cfg.NET_TYPE = "image"
    C.cfg.TRAIN.VGG16_EN = True

    def build_vgg():
        torch.manual_seed(7)                  # VGG16 keeps its constructor's initialisation, like tools/vgg16_bench.py
        net = V.vgg16()
        net.create_architecture(2, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
        net._device = dev
        net.to(dev)
        net.train()
        return net

    if not args.no_fc6:
        net = build_vgg()
        net._mode = 'TRAIN'
        hip_modules.set_net_mode('TRAIN')
        params = [p for p in net.vgg.classifier.parameters()]
        pooled = rand(ROIS, 7, 7, 512).permute(0, 3, 1, 2).requires_grad_(True)       # NCHW-shaped view of NHWC storage
        cot = rand(ROIS, 4096) - 0.5
        accumulate = autograd_ops.WgradSchedule(accumulate=True, side_stream=False, grouped=True, bn_stat_sink=None)
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()
        peak = {}

        def form(nchw, acc):
            def window():
                V.FC6_NCHW_FLATTEN = nchw
                for p in params:
                    p.grad = torch.zeros_like(p) if acc else None
                pooled.grad = None
                net.set_uc_seed(1)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                with autograd_ops.wgrad_schedule(accumulate if acc else autograd_ops.EAGER_SCHEDULE):
                    out = net._head_to_tail(pooled)
                    (out * cot).sum().backward()
                    autograd_ops.join_weight_grads(dev)
                b.record()
                b.synchronize()
                peak[(nchw, acc)] = torch.cuda.max_memory_allocated() - base
                return a.elapsed_time(b) * 1e-3
            return window
        forms = {(nchw, acc): form(nchw, acc) for acc in (False, True) for nchw in (True, False)}
        t = alternate(forms, max(args.reps // 3, 5), 2)
        V.FC6_NCHW_FLATTEN = True
        lines += ["", "## (b) fc6's filter gradient: NCHW flattening against the permuted filter, %d RoIs" % ROIS, "",
                  "relu(fc6) -> dropout -> relu(fc7) -> dropout forward and backward on a (%d,512,7,7) pooled tensor (an NCHW-shaped "
                  "view of NHWC storage, as RoIAlign returns it), device events around one forward + backward, ms; median (minimum - "
                  "maximum) of %d windows, the four forms alternating.  `eager`: the filter gradients go back to autograd (first "
                  "step: they become `param.grad`).  `accumulating`: the schedule of a captured step - this package's launches add "
                  "into existing `param.grad`, in line.  Peak: the highest device memory during the window above what was "
                  "allocated when it began (parameters, gradients, derived filters)." % (ROIS, max(args.reps // 3, 5)), "",
                  "| fc6 route | schedule | ms per forward + backward | peak MB above the resident set |", "|---|---|---|---|"]
        for (nchw, acc), v in t.items():
            lines.append("| %s | %s | %s | %.0f |" % ("NCHW flatten + `linear_train`" if nchw else "NHWC flatten + permuted filter",
                                                     "accumulating" if acc else "eager", spread(v, 1e3), peak[(nchw, acc)] / 1e6))
            print(lines[-1], flush=True)
        lines += ["", "Resident before the windows (parameters and the derived filters of the warm-up): %.0f MB." % (resident / 1e6)]
        hip_modules.set_net_mode(None)
        del net, params, pooled, cot
        torch.cuda.empty_cache()

    if not args.no_steps:
        import bench_configs as B
        from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
        from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
        h, w = 600, 1000
        rng = np.random.default_rng(3)
        blobs = {"data": (rng.standard_normal((1, h, w, 3)) * 50).astype(np.float32),
                 "info": np.array([0, w, 0, h, 0, 0, 1.0], np.float32),
                 "gt_boxes": np.array([[100, 80, 420, 380, 1], [520, 150, 900, 560, 1], [300, 300, 620, 590, 1]], np.float32),
                 "gt_boxes_dc": np.zeros((0, 4), np.float32)}
        lines += ["", "## (c) The training step, 1000 x 600, 2 classes, 3 boxes, 256 sampled RoIs", "",
                  "Host clock around %d steps that end in a device synchronise (a weight update every 16 frames), per step; "
                  "median of 3 windows after 8 untimed steps (tools/bench_configs.py's windows).  VGG16: the constructor's "
                  "initialisation, both dropouts live, its convolution plans tuned by the captured step's warm-up; ResNet-101 "
                  "without FPN: seeded weights, cfg.RESNET.FIXED_BLOCKS = 1.  Memory: allocated after the windows / the peak "
                  "during them." % args.steps, "",
                  "| net | mode | ms per step | steps/s | allocated MB | peak MB |", "|---|---|---|---|---|---|"]
        for name in ["VGG16"] + ([] if args.no_resnet else ["ResNet-101"]):
            def build():
                if name == "VGG16":
                    net = build_vgg()
                else:
                    torch.manual_seed(1)
                    net = imagenet(num_layers=101)
                    net.create_architecture(2, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
                    net.load_state_dict(seeded_state_dict(net, 7, bn_mode="tame"), strict=True)
                    net._device = dev
                    net.to(dev)
                    net.train()
                return net, torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)
            for mode in ("eager", "captured", "pipeline x%d" % args.inflight):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                net, opt = build()
                if mode == "eager":
                    _, dt = B._timed_train_windows(net, blobs, opt, args.steps)
                elif mode == "captured":
                    net.enable_train_graphs(True)
                    _, dt = B._timed_train_windows(net, blobs, opt, args.steps)
                else:
                    _, dt = B._timed_pipeline_windows(net, blobs, opt, args.steps, args.inflight)
                lines.append("| %s | %s | %.2f | %.1f | %.0f | %.0f |" % (name, mode, 1e3 * dt / args.steps, args.steps / dt,
                                                                      torch.cuda.memory_allocated() / 1e6,
                                                                      torch.cuda.max_memory_allocated() / 1e6))
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
