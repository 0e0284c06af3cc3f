#!/usr/bin/env python
"""Cost and accuracy of the split-bf16 convolution kernel (cfg.TEST.CONV_SPLIT_BF16, ``ops.conv2d_nhwc_bf16x3``) on the image
detector's 1000 x 600 frame (bench.py's net, weights and frames).  Same process, same device.

shapes  every distinct convolution of the frame with C % 32 == 0 (shape, residual operand, ReLU as the frame issues them,
        from ``ops.PROFILE`` of one eager frame with the switch off): ``ops.conv2d_nhwc`` under the tuned plan table
        profiles/r05_plans.json (a Winograd plan gets its pre-transformed filter) against ``ops.conv2d_nhwc_bf16x3`` under
        its tile rule and under each forced tile.  ``--inner`` back-to-back calls are captured into one hipGraph per form and
        stream.  alone: one replay between two device events.  four in flight: the same graph replayed on four streams at
        once (own output each), host clock around two device synchronisations, per call of one stream.  The forms
        alternate window by window, ``--reps`` windows each after ``--warmup``; median.
errors  post-ReLU normal activations, normal filters x Ktot^-1/2, no epilogue operands: largest and rms error of both
        kernels against the float64 convolution of the first image (computed on the device by unfold + matmul in float64).
frame   four captured frames on four streams per setting, as tools/conv_bf16_bench.py times them.

    python tools/conv_split_bf16_bench.py [--selected] [--no-frame] [--out FILE]

The table it prints is section 1 of profiles/conv_split_bf16.md, which adds the gate, the rule and the headline runs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def alternate(windows, reps, warmup):
    """windows: name -> callable returning seconds per unit.  Alternates them, drops the warm-up, returns name -> list."""
    out = {k: [] for k in windows}
    for r in range(warmup + reps):
        for k, fn in windows.items():
            t = fn()
            if r >= warmup:
                out[k].append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--selected", action="store_true", help="only the shapes the rule gives to the split kernel")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import bench
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model.streams import concurrent_streams
    from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device
    assert torch.cuda.is_available(), "conv_split_bf16_bench needs the MI355X"
    dev = "cuda:0"
    net, sd = bench.build_net(dev)
    cfg = C.cfg
    info = np.array([0, bench.W, 0, bench.H, 0, 0, 1.0], np.float32)
    with open(os.path.join(ROOT, "profiles", bench.PLANS_FILE)) as f:
        ops.import_conv_plans(json.load(f))
    frame = torch.from_numpy(bench.synthetic_frame(0)).to(dev)
    lanes = 4
    streams, _ = concurrent_streams(lanes, dev)

    # ---- the frame's eligible convolutions ------------------------------------------------------------------------------
    cfg.TEST.CONV_SPLIT_BF16 = False
    ops.PROFILE = []
    with torch.no_grad():
        detect_frame_device(net, frame, info, bench.THRESH, bench.MAX_DETS, bench.MAX_DETS)
    torch.cuda.synchronize()
    issued, ops.PROFILE = ops.PROFILE, None
    cfg.TEST.CONV_SPLIT_BF16 = True
    distinct = {}
    for p in issued:
        if p["c"] % 32 == 0:
            key = (p["n"], p["h"], p["w"], p["c"], p["k"], p["r"], p["s"], p["stride"], p["pad"], p["residual"], p["relu"])
            distinct[key] = distinct.get(key, 0) + 1
    lines = ["# Split-bf16 forward convolutions (`cfg.TEST.CONV_SPLIT_BF16`) against the tuned fp32 plans, shape by shape "
             "(`tools/conv_split_bf16_bench.py`)", "",
             "Reps %d, warm-up %d, %d calls per window." % (args.reps, args.warmup, args.inner), "",
             "%d of the %d convolutions of a 1000 x 600 frame have C %% 32 == 0 (%d distinct).  fp32: `ops.conv2d_nhwc` under "
             "profiles/%s (W = a Winograd plan, with its pre-transformed filter); split: `ops.conv2d_nhwc_bf16x3` under its tile "
             "rule (`alone`, `x4`) and under each forced tile (x4 only).  `alone`: device-event interval of one hipGraph replay of "
             "%d back-to-back calls, per call.  `x4`: the same graph on four streams at once, host clock, per call of one "
             "stream.  Median of %d windows, the forms alternating.  `rule` = `ops.conv_split_bf16_wanted`.  Errors: largest / rms "
             "against float64 on the first image, post-ReLU normal activations, normal filters."
             % (sum(distinct.values()), len(issued), len(distinct), bench.PLANS_FILE, args.inner, args.reps), "",
             "| n h w c k r stride | residual | calls | rule | fp32 alone us | split alone us | fp32 x4 us | split x4 us | fp32 / split x4 "
             "| split 64x64 x4 us | split 128x128 x4 us | split TFLOP/s x4 | fp32 max err | split max err | fp32 rms err | split rms err |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    g = torch.Generator().manual_seed(0)
    total = {"fp32": 0.0, "rule": 0.0}
    for key, calls in distinct.items():
        n, h, w, c, k, r, s, stride, pad, has_res, relu = key
        if args.selected and not ops.conv_split_bf16_wanted(n, h, w, c, k, r, s, stride, pad):
            continue
        ho, wo = ops.conv_out_hw(h, w, r, s, stride, pad)
        x = torch.randn((n, h, w, c), generator=g).clamp(min=0).to(dev)
        wt = (torch.randn((k, r, s, c), generator=g) * (r * s * c) ** -0.5).to(dev)
        scale, shift = torch.randn(k, generator=g).to(dev), torch.randn(k, generator=g).to(dev)
        res = torch.randn((n, ho, wo, k), generator=g).to(dev) if has_res else None
        ys = [torch.empty((n, ho, wo, k), device=dev) for _ in range(lanes)]
        u = ops.winograd_filter(wt) if (not has_res and ops.winograd_filter_wanted(n, h, w, c, k, r, s, stride, pad)) else None
        wp = ops.conv2d_pack_bf16x3(wt)
        wanted = ops.conv_split_bf16_wanted(n, h, w, c, k, r, s, stride, pad)
        # ---- accuracy: no epilogue operands, first image, float64 on the device
        cols = F.unfold(x[:1].permute(0, 3, 1, 2).double(), (r, s), padding=pad, stride=stride)[0]          # (c r s, L)
        ref = (wt.permute(0, 3, 1, 2).reshape(k, -1).double() @ cols).t()                                   # (L, k)
        del cols
        err = {}
        for name, call in (("fp32", lambda: ops.conv2d_nhwc(x, wt, stride=stride, pad=pad, w_winograd=u)),
                           ("split", lambda: ops.conv2d_nhwc_bf16x3(x, wp, stride=stride, pad=pad))):
            d = call()[0].reshape(-1, k).double() - ref
            err[name] = (float(d.abs().max()), float(d.pow(2).mean().sqrt()))
        del ref
        # ---- time
        forms = {"fp32": (lambda y: ops.conv2d_nhwc(x, wt, scale, shift, res, stride=stride, pad=pad, relu=relu, out=y, w_winograd=u), 0)}
        for name, tile in (("split", 0), ("split 64", 1), ("split 128", 2)):
            forms[name] = (lambda y: ops.conv2d_nhwc_bf16x3(x, wp, scale, shift, res, stride=stride, pad=pad, relu=relu, out=y), tile)
        graphs, first = {}, {}
        for name, (call, tile) in forms.items():
            ops.set_conv_bf16_tile(tile)
            first[name] = call(ys[0]).clone()
            torch.cuda.synchronize()
            graphs[name] = []
            for lane in range(lanes):
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for _ in range(args.inner):
                        call(ys[lane])
                graphs[name].append(gr)
        ops.set_conv_bf16_tile(0)
        assert torch.equal(first["split 64"], first["split 128"]) and torch.equal(first["split"], first["split 64"])
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())

        def alone(grs):
            def window():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                grs[0].replay()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e-3 / args.inner
            return window

        def loaded(grs):
            def window():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for lane in range(lanes):
                    with torch.cuda.stream(streams[lane]):
                        grs[lane].replay()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.inner
            return window
        ta = alternate({nm: alone(graphs[nm]) for nm in ("fp32", "split")}, args.reps, args.warmup)
        tl = alternate({nm: loaded(grs) for nm, grs in graphs.items()}, args.reps, args.warmup)
        ma = {nm: float(np.median(v)) for nm, v in ta.items()}
        ml = {nm: float(np.median(v)) for nm, v in tl.items()}
        flops = 2.0 * n * ho * wo * k * r * s * c
        total["fp32"] += calls * ml["fp32"]
        total["rule"] += calls * (ml["split"] if wanted else ml["fp32"])
        lines.append("| %d %d %d %d %d %d %d | %s | %d | %s | %.1f%s | %.1f | %.1f | %.1f | %.2f | %.1f | %.1f | %.0f | %.3g | %.3g | %.3g | %.3g |"
                     % (n, h, w, c, k, r, stride, "yes" if has_res else "no", calls, "yes" if wanted else "no", ma["fp32"] * 1e6,
                        " W" if u is not None else "", ma["split"] * 1e6, ml["fp32"] * 1e6, ml["split"] * 1e6, ml["fp32"] / ml["split"],
                        ml["split 64"] * 1e6, ml["split 128"] * 1e6, lanes * flops / ml["split"] * 1e-12, err["fp32"][0], err["split"][0],
                        err["fp32"][1], err["split"][1]))
        print(lines[-1], flush=True)
        del graphs
    lines += ["", "Sum over the frame's C %% 32 == 0 calls, four in flight (calls per frame x median): fp32 plans %.3f ms; with the "
              "rule's layers on the split kernel %.3f ms." % (total["fp32"] * 1e3, total["rule"] * 1e3)]

    # ---- four frames in flight ------------------------------------------------------------------------------------------
    if not args.no_frame:
        from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
        frames = [torch.from_numpy(bench.synthetic_frame(i)).to(dev) for i in range(5)]
        runners, dets = {}, {}
        for on in (False, True):
            cfg.TEST.CONV_SPLIT_BF16 = on
            runners[on] = [FrameRunner(net, bench.H, bench.W, bench.C, info, bench.THRESH, bench.MAX_DETS) for _ in range(lanes)]
            d, c_ = runners[on][0].run(frames[0])
            torch.cuda.synchronize()
            dets[on] = c_.cpu().tolist()
        cfg.TEST.CONV_SPLIT_BF16 = True
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())

        def frame_window(rs):
            def window():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.frames):
                    with torch.cuda.stream(streams[i % lanes]):
                        rs[i % lanes].run(frames[i % len(frames)])
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.frames
            return window
        t = alternate({on: frame_window(rs) for on, rs in runners.items()}, args.reps, args.warmup)
        med = {on: float(np.median(v)) for on, v in t.items()}
        lines += ["", "## Frames per second, 1000 x 600, four captured frames in flight", "",
                  "Four `FrameRunner`s per setting on four streams, frame i on stream i %% 4, %d frames per window between two "
                  "device synchronisations (host clock); median (best) of %d windows, the settings alternating on the same "
                  "device." % (args.frames, args.reps), "",
                  "| `cfg.TEST.CONV_SPLIT_BF16` | ms per frame | frames/s | detections per class (frame 0) |", "|---|---|---|---|"]
        for on in (False, True):
            lines.append("| %s | %.3f (%.3f) | %.1f | %s |" % ("on" if on else "off", med[on] * 1e3, min(t[on]) * 1e3, 1 / med[on], dets[on]))
        lines += ["", "Ratio of the medians, off / on: %.3f." % (med[False] / med[True])]
        del runners
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
