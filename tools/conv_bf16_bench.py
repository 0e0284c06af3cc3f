#!/usr/bin/env python
"""Cost and effect of cfg.TEST.CONV_BF16 on the image detector's 1000 x 600 frame (bench.py's net, weights and frames).
Same process, same device.

shapes  every distinct convolution of the frame with C % 32 == 0 (shape, residual operand, ReLU as the frame issues them,
        from ``ops.PROFILE`` of one eager frame): ``ops.conv2d_nhwc`` under the tuned plan table profiles/r05_plans.json
        (a Winograd plan gets its pre-transformed filter, as the net hands it over) against ``ops.conv2d_nhwc_bf16`` on
        the packed filter, random normal operands.  ``--inner`` back-to-back calls are captured into one hipGraph per
        form; a window is one replay between two device events; the two forms alternate window by window, ``--reps``
        windows each after ``--warmup``; median per call.  Device intervals, not a kernel trace: the gaps between the
        graph's kernel nodes are inside.  The bf16 column is also taken under each forced tile (64x64, 128x128).
frame   four captured frames (``model/frame_graph.FrameRunner``, filter included) on four streams per setting, frame i on
        stream i % 4 as bench.py drives them; a window is ``--frames`` frames between two host time stamps around device
        synchronisations; windows alternate between the settings.
agree   final detections on the structured-RPN frames of seeds 0 .. 7 (bench.py ``structured_rpn`` / ``map_delta``: injected
        RPN output, classifier weights x 8), switch on against switch off: a detection agrees when the other path holds a
        detection of the same class with IoU >= 0.7.

    python tools/conv_bf16_bench.py [--out profiles/conv_bf16.md]
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


def iou_matrix(a, b):
    x1, y1 = np.maximum(a[:, None, 0], b[None, :, 0]), np.maximum(a[:, None, 1], b[None, :, 1])
    x2, y2 = np.minimum(a[:, None, 2], b[None, :, 2]), np.minimum(a[:, None, 3], b[None, :, 3])
    inter = np.clip(x2 - x1 + 1, 0, None) * np.clip(y2 - y1 + 1, 0, None)
    area = lambda r: (r[:, 2] - r[:, 0] + 1) * (r[:, 3] - r[:, 1] + 1)
    return inter / (area(a)[:, None] + area(b)[None, :] - inter)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--no-agree", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device
    assert torch.cuda.is_available(), "conv_bf16_bench needs the MI355X"
    dev = "cuda:0"
    net, sd = bench.build_net(dev)
    cfg = C.cfg
    info = np.array([0, bench.W, 0, bench.H, 0, 0, 1.0], np.float32)
    with open(os.path.join(ROOT, "profiles", bench.PLANS_FILE)) as f:
        ops.import_conv_plans(json.load(f))
    frame = torch.from_numpy(bench.synthetic_frame(0)).to(dev)

    def timed_replay(graph, units):
        def window():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3 / units
        return window

    # ---- the frame's eligible convolutions ------------------------------------------------------------------------------
    ops.PROFILE = []
    with torch.no_grad():
        detect_frame_device(net, frame, info, bench.THRESH, bench.MAX_DETS, bench.MAX_DETS)
    torch.cuda.synchronize()
    issued, ops.PROFILE = ops.PROFILE, None
    distinct = {}
    for p in issued:
        if p["c"] % 32 == 0:
            key = (p["n"], p["h"], p["w"], p["c"], p["k"], p["r"], p["s"], p["stride"], p["pad"], p["residual"], p["relu"])
            distinct[key] = distinct.get(key, 0) + 1
    lines = ["# bf16-operand forward convolutions (`cfg.TEST.CONV_BF16`) against the fp32 path (`tools/conv_bf16_bench.py`)", "",
             "Command: `python tools/conv_bf16_bench.py --out profiles/conv_bf16.md` (reps %d, warm-up %d, %d calls per shape "
             "window, %d frames per frame window)." % (args.reps, args.warmup, args.inner, args.frames), "",
             "## The frame's convolutions with C % 32 == 0", "",
             "%d of the %d convolutions of a 1000 x 600 frame (%d distinct).  fp32: `ops.conv2d_nhwc` under "
             "profiles/%s (W = a Winograd plan, with its pre-transformed filter); bf16: `ops.conv2d_nhwc_bf16` under its tile "
             "rule, then under each forced tile.  Device-event interval of one hipGraph replay holding %d back-to-back calls, per "
             "call, median of %d windows, the forms alternating.  Random normal operands; the last column is the distance between the "
             "two forms' outputs on them (one layer of operand rounding; the three bf16 columns are bit-equal)."
             % (sum(distinct.values()), len(issued), len(distinct), bench.PLANS_FILE, args.inner, args.reps), "",
             "| n h w c k r stride | residual | calls per frame | fp32 us | bf16 us | fp32 / bf16 | bf16 64x64 us | bf16 128x128 us | fp32 TFLOP/s | bf16 TFLOP/s | relative L2 gap of the outputs |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    g = torch.Generator().manual_seed(0)
    total = {"fp32": 0.0, "bf16": 0.0}
    for key, calls in distinct.items():
        n, h, w, c, k, r, s, stride, pad, has_res, relu = key
        ho, wo = ops.conv_out_hw(h, w, r, s, stride, pad)
        x = torch.randn((n, h, w, c), generator=g).to(dev)
        wt = (torch.randn((k, r, s, c), generator=g) * (r * s * c) ** -0.5).to(dev)
        scale, shift = torch.randn(k, generator=g).to(dev), torch.randn(k, generator=g).to(dev)
        res = torch.randn((n, ho, wo, k), generator=g).to(dev) if has_res else None
        y = torch.empty((n, ho, wo, k), device=dev)
        u = ops.winograd_filter(wt) if (not has_res and ops.winograd_filter_wanted(n, h, w, c, k, r, s, stride, pad)) else None
        wp = ops.conv2d_pack_bf16(wt)
        forms = {"fp32": (lambda: ops.conv2d_nhwc(x, wt, scale, shift, res, stride=stride, pad=pad, relu=relu, out=y, w_winograd=u), 0)}
        for name, tile in (("bf16", 0), ("bf16 64", 1), ("bf16 128", 2)):
            forms[name] = (lambda: ops.conv2d_nhwc_bf16(x, wp, scale, shift, res, stride=stride, pad=pad, relu=relu, out=y), tile)
        graphs, first = {}, {}
        for name, (call, tile) in forms.items():
            ops.set_conv_bf16_tile(tile)
            first[name] = call().clone()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(args.inner):
                    call()
            graphs[name] = gr
        ops.set_conv_bf16_tile(0)
        t = alternate({nm: timed_replay(gr, args.inner) for nm, gr in graphs.items()}, args.reps, args.warmup)
        med = {nm: float(np.median(v)) for nm, v in t.items()}
        flops = 2.0 * n * ho * wo * k * r * s * c
        rel = float((first["bf16"] - first["fp32"]).double().norm() / first["fp32"].double().norm())
        assert torch.equal(first["bf16 64"], first["bf16 128"]) and torch.equal(first["bf16"], first["bf16 64"])
        total["fp32"] += calls * med["fp32"]
        total["bf16"] += calls * med["bf16"]
        lines.append("| %d %d %d %d %d %d %d | %s | %d | %.1f%s | %.1f | %.2f | %.1f | %.1f | %.1f | %.1f | %.2g |"
                     % (n, h, w, c, k, r, stride, "yes" if has_res else "no", calls, med["fp32"] * 1e6, " W" if u is not None else "",
                        med["bf16"] * 1e6, med["fp32"] / med["bf16"], med["bf16 64"] * 1e6, med["bf16 128"] * 1e6,
                        flops / med["fp32"] * 1e-12, flops / med["bf16"] * 1e-12, rel))
        del graphs
    lines += ["", "Sum over the frame's eligible calls (calls per frame x median): fp32 %.3f ms, bf16 %.3f ms, ratio %.2f."
              % (total["fp32"] * 1e3, total["bf16"] * 1e3, total["fp32"] / total["bf16"])]

    # ---- four frames in flight ------------------------------------------------------------------------------------------
    if not args.no_frame:
        from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
        from faster_rcnn_pytorch_multimodal_amd.model.streams import concurrent_streams
        lanes = 4
        streams, _ = concurrent_streams(lanes, dev)
        frames = [torch.from_numpy(bench.synthetic_frame(i)).to(dev) for i in range(5)]
        runners, dets = {}, {}
        for on in (False, True):
            cfg.TEST.CONV_BF16 = on
            runners[on] = [FrameRunner(net, bench.H, bench.W, bench.C, info, bench.THRESH, bench.MAX_DETS) for _ in range(lanes)]
            d, c_ = runners[on][0].run(frames[0])
            torch.cuda.synchronize()
            dets[on] = c_.cpu().tolist()
        cfg.TEST.CONV_BF16 = False
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
                  "| `cfg.TEST.CONV_BF16` | ms per frame | frames/s | detections per class (frame 0) |", "|---|---|---|---|"]
        for on in (False, True):
            lines.append("| %s | %.3f (%.3f) | %.1f | %s |" % ("on" if on else "off", med[on] * 1e3, min(t[on]) * 1e3, 1 / med[on], dets[on]))
        lines += ["", "Ratio of the medians, off / on: %.3f." % (med[False] / med[True])]
        del runners

    # ---- agreement of the final detections ------------------------------------------------------------------------------
    if not args.no_agree:
        sd8 = dict(sd)
        sd8["cls_score_net.weight"] = sd8["cls_score_net.weight"] * 8.0
        net.load_state_dict(sd8, strict=True)
        lines += ["", "## Final detections on the structured-RPN frames of seeds 0 .. 7", "",
                  "bench.py's `structured_rpn` output injected on both paths, classifier weights x 8 (as its `map_delta`), score "
                  "threshold %.1f, max_dets %d.  A detection agrees when the other path holds one of the same class with "
                  "IoU >= 0.7." % (bench.THRESH, bench.MAX_DETS), "",
                  "Boxes with x2 <= x1 or y2 <= y1 are dropped on both sides.  The last five columns compare the two paths RoI by "
                  "RoI BEFORE the per-class NMS (same proposals on both paths): RoIs whose class-1 score is above the threshold on "
                  "both paths, RoIs above it on one path only, the smallest IoU between the two paths' class-1 boxes of one RoI "
                  "(RoIs above the threshold with a valid box on both paths), and the largest class-1 score gap of a RoI above "
                  "the threshold.", "",
                  "| seed | fp32 detections | bf16 detections | fp32 found in bf16 | bf16 found in fp32 | largest score gap of the matched "
                  "| RoIs | above the threshold on both | on one path only | smallest box IoU of one RoI | largest score gap |",
                  "|---|---|---|---|---|---|---|---|---|---|---|"]
        tot = [0, 0, 0, 0]
        valid = lambda b: b[(b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])]      # (bench.py map_delta drops the same boxes)
        for seed in range(8):
            f = torch.from_numpy(bench.synthetic_frame(seed)).to(dev)
            cls, box = bench.structured_rpn(seed)
            net._rpn_override = bench.fuse_rpn(cls, box).to(dev)
            got = {}
            try:
                for on in (False, True):
                    cfg.TEST.CONV_BF16 = on
                    with torch.no_grad():
                        d, c_ = detect_frame_device(net, f, info, bench.THRESH, bench.MAX_DETS, bench.MAX_DETS)
                    torch.cuda.synchronize()
                    pr = net._predictions
                    nr = int(pr["rois_count"].item())
                    got[on] = (d.cpu().numpy(), c_.cpu().numpy(), pr["rois"][:nr].cpu().numpy(),
                               pr["pred_boxes"][:nr].cpu().numpy().astype(np.float64), pr["cls_prob"][:nr].cpu().numpy())
            finally:
                net._rpn_override = None
                cfg.TEST.CONV_BF16 = False
            na = nb = fa = fb = 0
            gap = 0.0
            for j in range(1, bench.NUM_CLASSES):
                a, b = valid(got[False][0][j, :got[False][1][j]]), valid(got[True][0][j, :got[True][1][j]])
                na, nb = na + len(a), nb + len(b)
                if len(a) and len(b):
                    m = iou_matrix(a[:, :4].astype(np.float64), b[:, :4].astype(np.float64))
                    fa += int((m.max(1) >= 0.7).sum())
                    fb += int((m.max(0) >= 0.7).sum())
                    hit = m.max(1) >= 0.7
                    if hit.any():
                        gap = max(gap, float(np.abs(a[hit, 4] - b[m.argmax(1)[hit], 4]).max()))
            tot = [tot[0] + na, tot[1] + nb, tot[2] + fa, tot[3] + fb]
            # RoI by RoI (the injected RPN output gives both paths the same proposals): class-1 box and score of RoI i
            same_rois = got[False][2].shape == got[True][2].shape and bool((got[False][2] == got[True][2]).all())
            if same_rois:
                sa, sb = got[False][4][:, 1], got[True][4][:, 1]
                ba, bb = got[False][3][:, 4:8], got[True][3][:, 4:8]
                above = (sa > bench.THRESH) & (sb > bench.THRESH)
                side = int(((sa > bench.THRESH) != (sb > bench.THRESH)).sum())
                ok = above & (ba[:, 2] > ba[:, 0]) & (ba[:, 3] > ba[:, 1]) & (bb[:, 2] > bb[:, 0]) & (bb[:, 3] > bb[:, 1])
                x1, y1 = np.maximum(ba[:, 0], bb[:, 0]), np.maximum(ba[:, 1], bb[:, 1])
                x2, y2 = np.minimum(ba[:, 2], bb[:, 2]), np.minimum(ba[:, 3], bb[:, 3])
                inter = np.clip(x2 - x1 + 1, 0, None) * np.clip(y2 - y1 + 1, 0, None)
                area = lambda r: (r[:, 2] - r[:, 0] + 1) * (r[:, 3] - r[:, 1] + 1)
                iou = (inter / (area(ba) + area(bb) - inter))[ok]
                per_roi = "%d | %d | %d | %s | %.2g" % (len(sa), int(above.sum()), side, ("%.4f" % iou.min()) if len(iou) else "-",
                                                        float(np.abs(sa - sb)[above | (sa > bench.THRESH) | (sb > bench.THRESH)].max(initial=0.0)))
            else:
                per_roi = "proposals differ | | | |"
            lines.append("| %d | %d | %d | %d | %d | %.2g | %s |" % (seed, na, nb, fa, fb, gap, per_roi))
        lines += ["", "All seeds: %d of %d fp32 detections have a bf16 partner (%.1f %%), %d of %d bf16 detections an fp32 partner (%.1f %%)."
                  % (tot[2], tot[0], 100.0 * tot[2] / max(tot[0], 1), tot[3], tot[1], 100.0 * tot[3] / max(tot[1], 1))]
        net.load_state_dict(sd, strict=True)
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
