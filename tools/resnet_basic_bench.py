#!/usr/bin/env python
"""The closing convolution of a BasicBlock (conv2 + bn2 + identity + ReLU) three ways, and the ResNet-34 frame.  Same process,
same device.

(a) conv2   every distinct ``conv2`` shape of a 1000 x 600 ResNet-34 frame with 300 RoIs (layer1 150 x 250 x 64, layer2
            75 x 125 x 128, layer3 38 x 63 x 256, layer4 300 x 7 x 7 x 512), each with folded BatchNorm, residual and ReLU:
              fused      ``ops.conv2d_nhwc_winograd_res`` on the Winograd plan the autotuner picks for the residual-free call of
                         the shape (tuned under ``set_conv_algo(2)``: the best Winograd plan), pre-transformed filter;
              gemm       ``ops.conv2d_nhwc(residual=...)`` on the plan the autotuner picks under the residual key: the
                         implicit GEMM with the residual in its epilogue, the only single-launch route before this kernel;
              unfused    the residual-free Winograd call (the same plan as `fused`, relu off) followed by ``torch.relu(y + res)``
                         (two element-wise launches over the map);
              split-bf16 where the library's rule gives the shape to ``ops.conv2d_nhwc_bf16x3`` (cfg.TEST.CONV_SPLIT_BF16,
                         default on, comes BEFORE the fp32 routes in ``hip_modules.conv_forward``), that call with the residual.
            ``--inner`` back-to-back calls are captured into one hipGraph over a ring of operand sets; a window is one replay
            between two device events; the routes alternate window by window.  Also the plan the autotuner would pick for
            the residual-free call with both forms allowed (``set_conv_algo(0)``): where that is the implicit GEMM, the new
            entry point runs the GEMM with the residual - the shape stays on `gemm`.
(b) frame   the captured ResNet-34 frame (``model/frame_graph.FrameRunner``: 1000 x 600, 300 proposals, 2 classes, filter
            included; its convolution plans tuned by the runner's warm-up frames) with one and with four frames in flight, and
            the ResNet-101 frame of the same process beside it (plans from the committed table).

    python tools/resnet_basic_bench.py [--out profiles/resnet_basic.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

RING_BYTES = 640 << 20       # a ring grows towards this footprint (2.5 x the 256 MiB Infinity Cache), up to --inner sets
# (name, n, h, w, c): conv2 is c -> c, 3x3 / stride 1 / pad 1
CONV2 = [("layer1", 1, 150, 250, 64), ("layer2", 1, 75, 125, 128), ("layer3", 1, 38, 63, 256), ("layer4", 300, 7, 7, 512)]


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
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--no-convs", action="store_true")
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    assert torch.cuda.is_available(), "resnet_basic_bench needs the MI355X"
    dev = "cuda:0"
    lib = _hip.load()
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
        calls[0]()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for c in calls:
                c()
        return graph

    def plan_of(n, h, w, c, residual):
        key = [n, h, w, c, c, 3, 3, 1, 1, 1 + (256 if residual else 0)]
        for row in ops.export_conv_plans():
            if row[:10] == key:
                code, tile = row[10] >> 4, row[10] & 15
                form = ("GEMM", "Winograd", "Winograd, fused input transform")[code]
                return "%s, tile %d%s" % (form, tile, ", %d splits" % row[11] if row[11] > 1 else "")
        return "none"

    lines = ["# BasicBlock ResNets: the residual Winograd output transform and the ResNet-34 frame (`tools/resnet_basic_bench.py`)",
             "", "Command: `python tools/resnet_basic_bench.py --out profiles/resnet_basic.md` (reps %d, warm-up %d, %d calls per "
             "call window, %d frames per frame window)." % (args.reps, args.warmup, args.inner, args.frames)]

    if not args.no_convs:
        lines += ["", "## (a) conv2 + bn2 + identity + ReLU of a 1000 x 600 ResNet-34 frame, 300 RoIs", "",
                  "Device-event interval of one hipGraph replay holding %d back-to-back calls over a ring of operand sets, per "
                  "call; median (minimum) of %d windows, the routes alternating.  `fused`: the new entry point on the tuned "
                  "Winograd plan; `gemm`: the implicit GEMM with the residual on its tuned plan; `unfused`: residual-free Winograd "
                  "on the same plan as `fused`, then `torch.relu(y + res)`; `split-bf16`: only where the library's rule takes the "
                  "shape (it then runs BEFORE any fp32 route in the net).  `plan, both forms allowed`: what the autotuner picks for "
                  "the residual-free call under `set_conv_algo(0)` - `GEMM` there means the net's call stays on the residual GEMM."
                  % (args.inner, args.reps), "",
                  "| conv2 | M x 9C -> K | GFLOP | fused us | gemm us | unfused us | split-bf16 us | fused / gemm | fused / unfused | Winograd plan | GEMM plan | plan, both forms allowed |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        with torch.no_grad():
            for name, n, h, w, c in CONV2:
                k = c
                wt = (torch.randn((k, 3, 3, c), device=dev, generator=g) * float(np.sqrt(2.0 / (9 * c)))).contiguous()
                scale = 0.5 + torch.rand((k,), device=dev, generator=g)
                shift = torch.rand((k,), device=dev, generator=g) * 0.2 - 0.1
                u = ops.winograd_filter(wt)
                nbytes = 4 * n * h * w * (c + 2 * k)
                sets = int(min(args.inner, max(1, -(-RING_BYTES // nbytes))))
                xs = [torch.randn((n, h, w, c), device=dev, generator=g) for _ in range(sets)]
                rs = [torch.randn((n, h, w, k), device=dev, generator=g) for _ in range(sets)]
                ys = [torch.empty((n, h, w, k), device=dev) for _ in range(sets)]
                # plans: both forms allowed (for the record), then the best Winograd plan under the residual-free key and the best
                # GEMM plan under the residual key
                _hip.check(lib.frcnn_conv2d_clear_plans(), "clear_plans")
                ops.set_conv_autotune(True)
                ops.set_conv_algo(0)
                ops.conv2d_nhwc(xs[0], wt, scale, shift, None, stride=1, pad=1, relu=True, w_winograd=u)
                both = plan_of(n, h, w, c, False)
                _hip.check(lib.frcnn_conv2d_clear_plans(), "clear_plans")
                ops.set_conv_algo(2)
                ops.conv2d_nhwc_winograd_res(xs[0], wt, rs[0], scale, shift, relu=True, w_winograd=u)
                ops.set_conv_algo(0)
                ops.conv2d_nhwc(xs[0], wt, scale, shift, rs[0], stride=1, pad=1, relu=True)
                ops.set_conv_autotune(False)
                torch.cuda.synchronize()
                assert ops.conv_plan_algo(n, h, w, c, k, 3, 3, 1, 1, False) == 1 and ops.conv_plan_algo(n, h, w, c, k, 3, 3, 1, 1, True) == 0
                routes = {
                    "fused": lambda i: ops.conv2d_nhwc_winograd_res(xs[i], wt, rs[i], scale, shift, relu=True, out=ys[i], w_winograd=u),
                    "gemm": lambda i: ops.conv2d_nhwc(xs[i], wt, scale, shift, rs[i], stride=1, pad=1, relu=True, out=ys[i]),
                    "unfused": lambda i: torch.relu(ops.conv2d_nhwc(xs[i], wt, scale, shift, None, stride=1, pad=1, relu=False, out=ys[i],
                                                                    w_winograd=u) + rs[i]),
                }
                if c % 32 == 0 and ops.conv_split_bf16_wanted(n, h, w, c, k, 3, 3, 1, 1):
                    packed = ops.conv2d_pack_bf16x3(wt)
                    routes["split-bf16"] = lambda i: ops.conv2d_nhwc_bf16x3(xs[i], packed, scale, shift, rs[i], stride=1, pad=1, relu=True, out=ys[i])
                a = routes["fused"](0).clone()
                b = routes["unfused"](0)
                torch.cuda.synchronize()
                assert torch.equal(a, b), "fused and unfused differ"
                graphs = {r: captured([(lambda i=i, fn=fn: fn(i % sets)) for i in range(args.inner)]) for r, fn in routes.items()}
                t = alternate({r: timed_replay(gr, args.inner) for r, gr in graphs.items()}, args.reps, args.warmup)
                med = {r: float(np.median(v)) for r, v in t.items()}
                cell = lambda r: "%.1f (%.1f)" % (med[r] * 1e6, min(t[r]) * 1e6) if r in med else "-"
                flops = 2.0 * n * h * w * k * 9 * c
                lines.append("| %s (%d,%d,%d,%d) | %d x %d -> %d | %.1f | %s | %s | %s | %s | %.2f | %.2f | %s | %s | %s |"
                             % (name, n, h, w, c, n * h * w, 9 * c, k, flops / 1e9, cell("fused"), cell("gemm"), cell("unfused"),
                                cell("split-bf16"), med["fused"] / med["gemm"], med["fused"] / med["unfused"],
                                plan_of(n, h, w, c, False), plan_of(n, h, w, c, True), both))
                del graphs, xs, rs, ys
                torch.cuda.empty_cache()
        _hip.check(lib.frcnn_conv2d_clear_plans(), "clear_plans")

    if not args.no_frame:
        from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
        from faster_rcnn_pytorch_multimodal_amd.model.streams import concurrent_streams
        from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
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
        nets = {"ResNet-34": imagenet(num_layers=34), "ResNet-101": imagenet(num_layers=101)}
        runners, rois, routes34 = {}, {}, None
        for name, net in nets.items():
            net.create_architecture(2, tag="default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
            net.load_state_dict(seeded_state_dict(net, 7, bn_mode="tame"), strict=True)
            net.eval()
            net._device = dev
            net.to(dev)
            runners[name] = []
            for i, s in enumerate(streams):
                with torch.cuda.stream(s):
                    # ResNet-34's shapes are in no committed table: the first runner's warm-up frames tune them
                    runners[name].append(FrameRunner(net, h, w, 3, info, thresh=0.05, max_dets=100,
                                                     autotune=(name == "ResNet-34" and i == 0)))
                torch.cuda.synchronize()
            runners[name][0].run(blob)
            torch.cuda.synchronize()
            rois[name] = int(runners[name][0].predictions["rois_count"].item())
            if name == "ResNet-34":
                routes34 = [(nm, plan_of(n, hh, ww, c, False), bool(ops.conv_split_bf16_wanted(n, hh, ww, c, c, 3, 3, 1, 1)))
                            for nm, n, hh, ww, c in CONV2]

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
        lines += ["", "## (b) The captured frame, 1000 x 600, 2 classes", "",
                  "One captured frame per stream (filter included); host clock around %d replays that end in a device "
                  "synchronise, per frame; median (minimum) of %d windows, the nets alternating.  Seeded weights.  ResNet-101: the "
                  "convolution plans of the committed table; ResNet-34: plans tuned by its first runner's warm-up frames."
                  % (args.frames, args.reps), "",
                  "| net | proposals | frames in flight | ms per frame | frames/s |", "|---|---|---|---|---|"]
        for lanes in (1, 4):
            t = alternate({name: frame_window(rs, lanes) for name, rs in runners.items()}, args.reps, args.warmup)
            for name, v in t.items():
                med = float(np.median(v))
                lines.append("| %s | %d | %d | %.3f (%.3f) | %.1f |" % (name, rois[name], lanes, med * 1e3, min(v) * 1e3, 1 / med))
        lines += ["", "Route of ResNet-34's conv2 calls in that frame (the plan tuned under the residual-free key; `split-bf16` = the "
                  "library's rule takes the shape before any fp32 route): "
                  + "; ".join("%s: %s%s" % (nm, pl, ", split-bf16" if sb else "") for nm, pl, sb in routes34) + "."]
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
