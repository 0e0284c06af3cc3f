#!/usr/bin/env python
"""The wide detection tail (``ops.head_softmax_decode_wide``) alone and inside the captured frame.  Same process, same device.

(a) tail    R = 300, C = 2048; image K = 21, 81; LiDAR K = 9, 11.  Beside it the composition that runs these shapes without
            the kernel: ``F.linear`` x 2, ``torch.softmax``, ``raw * stds + means`` and ``ops.bbox_transform_inv`` /
            ``ops.lidar_bbox_transform_inv``.  Two clocks, the two sides alternating:
              eager   one call between two device events, median (minimum) of ``--calls`` calls - what the issue of the
                      host's launches costs is inside (2 kernel launches against 6);
              graph   ``--inner`` back-to-back calls captured into one hipGraph, one replay between two device events, per
                      call - the device time alone.
            Weight bytes: a workgroup of the GEMM reads its half of the channels of its 32 weight rows once, so a call reads
            (K + E K) * C * 4 bytes per RoI tile of 32 - the minimum of a tiling that does not keep weights across RoI tiles;
            the fused kernel's form would read that once per RoI.  The column is computed from the launch geometry, not
            counted.
(b) tiles   what one launch instead of two would cost: a workgroup that owns all columns of its 32 RoIs runs the column
            tiles of a row one after the other.  R = 32 with K = 81 (13 column tiles side by side), with K = 6 (one tile) and
            R = 300 with K = 81 (130 tiles), graph clock.
(c) frame   the captured 1000 x 600 ResNet-101 frame (``FrameRunner``, filter included) at ``bench.NUM_CLASSES``, 21 and 81
            classes, one and four frames in flight; and, on the K-class frame's own tensors, the tail and the per-class filter
            alone (graph clock) - which of the two grows with K.

    python tools/head_wide_bench.py [--out profiles/head_wide.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

TAIL_SHAPES = [("image", 300, 2048, 21), ("image", 300, 2048, 81), ("lidar", 300, 2048, 9), ("lidar", 300, 2048, 11)]
TILE_SHAPES = [("image", 32, 2048, 6), ("image", 32, 2048, 81), ("image", 300, 2048, 81)]
NORM = {"image": ([0.1, 0.1, 0.2, 0.2], [0.0] * 4), "lidar": ([0.1, 0.1, 0.1, 0.2, 0.2, 0.2, 1.0], [0.0] * 7)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import bench
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    assert torch.cuda.is_available(), "head_wide_bench needs the MI355X"
    dev = "cuda:0"
    C.reset_cfg()
    C.cfg.NET_TYPE = "image"
    g = torch.Generator(device=dev).manual_seed(5)

    def event_time(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def alternate(fns, reps, warmup, units=1):
        out = {k: [] for k in fns}
        for r in range(warmup + reps):
            for k, fn in fns.items():
                t = event_time(fn) / units
                if r >= warmup:
                    out[k].append(t)
        return {k: (float(np.median(v)), float(min(v))) for k, v in out.items()}

    def captured(fn, inner):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            keep = [fn() for _ in range(inner)]
        graph.keep = keep
        return graph

    def tail_case(form, r, c, k):
        e = 4 if form == "image" else 7
        stds, means = NORM[form]
        fc7 = torch.rand((r, c), device=dev, generator=g) + 0.1
        wc = torch.randn((k, c), device=dev, generator=g) / float(np.sqrt(c))
        wb = torch.randn((e * k, c), device=dev, generator=g) / float(np.sqrt(c))
        bc, bb = torch.zeros(k, device=dev), torch.zeros(e * k, device=dev)
        xy = torch.rand((r, 2), device=dev, generator=g) * 500
        rois = torch.cat((torch.zeros((r, 1), device=dev), xy, xy + 20 + torch.rand((r, 2), device=dev, generator=g) * 200), 1).contiguous()
        anchors = (torch.randn((r, 7), device=dev, generator=g).abs() + 0.5).contiguous() if e == 7 else None
        boxes = rois[:, 1:5].contiguous()
        stds_t, means_t = torch.tensor(stds, device=dev).repeat(k), torch.tensor(means, device=dev).repeat(k)

        def wide():
            return ops.head_softmax_decode_wide(fc7, wc, bc, wb, bb, rois, stds, means, 1.0, roi_anchors_3d=anchors)

        def composed():
            score = F.linear(fc7, wc, bc)
            prob = torch.softmax(score, 1)
            raw = F.linear(fc7, wb, bb)
            deltas = raw * stds_t + means_t
            pred = (ops.bbox_transform_inv(boxes, deltas, 1.0) if e == 4 else
                    ops.lidar_bbox_transform_inv(boxes, anchors, deltas, 1.0))
            return score, prob, raw, pred
        out, (score, prob, raw, pred) = wide(), composed()
        gap = max(float((out["cls_prob"] - prob).abs().max()),
                  float(((out["pred_boxes"] - pred).abs() / pred.abs().clamp_min(1.0)).max()))
        assert gap < 1e-4, "the two sides disagree: %g" % gap
        return wide, composed, e

    lines = ["# The wide detection tail (`tools/head_wide_bench.py`)", "",
             "Command: `python tools/head_wide_bench.py --out profiles/head_wide.md` (eager clock: %d calls after %d warm-up "
             "calls; graph clock: %d calls per replay, %d replays; the two sides alternate call by call)."
             % (args.calls, args.warmup, args.inner, args.calls)]
    lines += ["", "## (a) The tail alone, R = 300, C = 2048", "",
              "`wide`: `ops.head_softmax_decode_wide` (2 launches).  `composed`: `F.linear` x 2, `torch.softmax`, "
              "`raw * stds + means`, `ops.(lidar_)bbox_transform_inv` (6 launches) - what runs these shapes without the kernel.  "
              "us per call, median (minimum).  Weight bytes per call: (K + E K) * C * 4 per RoI tile of 32 RoIs, from the launch "
              "geometry; `x minimum` is that over one pass over the weights per RoI tile (1.00 by construction: a workgroup "
              "reads its half of the channels of its 32 weight rows once and nothing is read twice inside a RoI tile); `fused form` is what one workgroup per "
              "RoI would read.", "",
              "| form | K | outputs | wide eager | composed eager | wide graph | composed graph | composed / wide (graph) | weight MB per call | x minimum | fused form MB |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    verdict = []
    for form, r, c, k in TAIL_SHAPES:
        wide, composed, e = tail_case(form, r, c, k)
        eager = alternate({"wide": wide, "composed": composed}, args.calls, args.warmup)
        graphs = {"wide": captured(wide, args.inner), "composed": captured(composed, args.inner)}
        graph = alternate({n: gr.replay for n, gr in graphs.items()}, args.calls, args.warmup, args.inner)
        n_out = k * (1 + e)
        tiles = -(-r // 32)
        wbytes = n_out * c * 4 * tiles
        ratio = graph["composed"][0] / graph["wide"][0]
        verdict.append((form, k, ratio, eager["composed"][0] / eager["wide"][0]))
        us = lambda t: "%.1f (%.1f)" % (t[0] * 1e6, t[1] * 1e6)
        lines.append("| %s | %d | %d | %s | %s | %s | %s | %.2f | %.1f | 1.00 | %.0f |"
                     % (form, k, n_out, us(eager["wide"]), us(eager["composed"]), us(graph["wide"]), us(graph["composed"]), ratio,
                        wbytes / 1e6, n_out * c * 4 * r / 1e6))
        del graphs
    lines += ["", "Not slower than the composition on either clock: " + "; ".join(
        "%s K = %d: %s (graph %.2fx, eager %.2fx)" % (f_, k, "yes" if min(a, b) >= 1.0 else "NO", a, b) for f_, k, a, b in verdict) + "."]

    lines += ["", "## (b) One launch or two", "",
              "Graph clock, us per call (both launches).  A single-launch form needs a workgroup that owns every column of its "
              "RoIs, i.e. one workgroup per 32 RoIs running its column tiles one after the other; the first two rows give the "
              "time of one column tile and of 13 of them side by side (each tile's channels split over two workgroups).", "",
              "| R | K | GEMM workgroups (columns x rows x channel halves) | us per call |", "|---|---|---|---|"]
    for form, r, c, k in TILE_SHAPES:
        wide, _, e = tail_case(form, r, c, k)
        gr = captured(wide, args.inner)
        t = alternate({"wide": gr.replay}, args.calls, args.warmup, args.inner)["wide"]
        lines.append("| %d | %d | %d x %d x 2 | %.1f (%.1f) |" % (r, k, -(-k * (1 + e) // 32), -(-r // 32), t[0] * 1e6, t[1] * 1e6))
        del gr

    if not args.no_frame:
        from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
        from faster_rcnn_pytorch_multimodal_amd.model.streams import concurrent_streams
        from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
        from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
        h, w = 600, 1000
        info = np.array([0, w, 0, h, 0, 0, 1.0], np.float32)
        blob = torch.from_numpy(bench.synthetic_frame(3)).to(dev)
        streams, _ = concurrent_streams(4, torch.device(dev))
        plans = os.path.join(ROOT, "profiles", bench.PLANS_FILE)
        if os.path.exists(plans):
            with open(plans) as f:
                ops.import_conv_plans(json.load(f))
        class_counts = sorted({int(bench.NUM_CLASSES), 21, 81})
        runners, parts = {}, {}
        for k in class_counts:
            net = imagenet(num_layers=101)
            net.create_architecture(k, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
            net.load_state_dict(seeded_state_dict(net, 7, bn_mode="tame"), strict=True)
            net.eval()
            net._device = dev
            net.to(dev)
            thresh = 1.0 / k          # a uniform softmax sits at 1 / K: about half of the scores pass, at every K
            runners[k] = []
            for s in streams:
                with torch.cuda.stream(s):
                    runners[k].append(FrameRunner(net, h, w, 3, info, thresh=thresh, max_dets=bench.MAX_DETS, autotune=False))
                torch.cuda.synchronize()
            dets, counts = runners[k][0].run(blob)
            torch.cuda.synchronize()
            p = runners[k][0].predictions
            fc7, rois = p["_tail"]["fc7"].clone(), p["rois"].clone()
            cls_prob, pred_boxes = p["cls_prob"].clone(), p["pred_boxes"].clone()
            tail = lambda net=net, fc7=fc7, rois=rois: net._tail_kernel(fc7.view(fc7.shape[0], 1, 1, -1), rois)
            filt = lambda cls_prob=cls_prob, pred_boxes=pred_boxes, thresh=thresh: ops.filter_per_class(
                pred_boxes, cls_prob, float(w), float(h), 1.0, thresh, float(C.cfg.TEST.NMS_THRESH), bench.MAX_DETS, bench.MAX_DETS)
            g_tail, g_filt = captured(tail, args.inner), captured(filt, args.inner)
            t = alternate({"tail": g_tail.replay, "filter": g_filt.replay}, args.calls, args.warmup, args.inner)
            parts[k] = (t["tail"], t["filter"], int(p["rois_count"].item()), int(counts.sum().item()), thresh)
            del g_tail, g_filt

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
        lines += ["", "## (c) The captured 1000 x 600 ResNet-101 frame", "",
                  "One captured frame per stream, filter included; host clock around %d replays that end in a device "
                  "synchronise, per frame; median (minimum) of %d windows, the class counts alternating.  Seeded weights, the "
                  "committed convolution plans, score threshold 1 / K (a seeded head's softmax is close to uniform, so about "
                  "half of the scores pass at every K), max_dets %d.  K = %d is `bench.NUM_CLASSES` and takes the fused tail; 21 "
                  "and 81 take the wide one." % (args.frames, args.reps, bench.MAX_DETS, bench.NUM_CLASSES), "",
                  "| K | frames in flight | ms per frame | frames/s |", "|---|---|---|---|"]
        for lanes in (1, 4):
            res = {k: [] for k in class_counts}
            for r in range(args.reps + 2):
                for k in class_counts:
                    v = frame_window(runners[k], lanes)()
                    if r >= 2:
                        res[k].append(v)
            for k in class_counts:
                med = float(np.median(res[k]))
                lines.append("| %d | %d | %.3f (%.3f) | %.1f |" % (k, lanes, med * 1e3, min(res[k]) * 1e3, 1 / med))
        lines += ["", "The tail and the per-class filter alone on that frame's own tensors (graph clock, us per call):", "",
                  "| K | tail | proposals | threshold | detections kept | tail us | filter us |", "|---|---|---|---|---|---|---|"]
        for k in class_counts:
            tl, fl, n, kept, thresh = parts[k]
            lines.append("| %d | %s | %d | %.4f | %d | %.1f (%.1f) | %.1f (%.1f) |"
                         % (k, "wide" if ops.head_uses_wide_form(k, 4) else "fused", n, thresh, kept, tl[0] * 1e6, tl[1] * 1e6,
                            fl[0] * 1e6, fl[1] * 1e6))
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
