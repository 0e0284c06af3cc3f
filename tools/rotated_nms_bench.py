#!/usr/bin/env python
"""Cost of cfg.TEST.NMS_ROTATED: the LiDAR per-class filter with the reference's yaw-less rule
(``frcnn_filter_per_class_lidar``) against the rotated rule (``frcnn_filter_per_class_lidar_rot``) on the same inputs, and
a LiDAR frame with the switch off and on.  Same process, same device.

filter  300 RoIs, 2 and 4 classes, a dense seeded prediction set: ceil(300 / 3) cars on a 30 x 20 m patch, each predicted
        about three times with jitter, a third of the predictions in the other anchor's form (l and w swapped,
        ry + pi/2); scores uniform in (0, 1), score threshold 0.1, NMS threshold cfg.TEST.NMS_THRESH, max_dets 100.
        ``--inner`` back-to-back calls are captured into one hipGraph per rule (kernel nodes only: no Python and no
        launch enqueue inside the timed region); a window is one replay between two device events; the two rules
        alternate window by window, ``--reps`` windows each after ``--warmup``; median and minimum per call.  Device
        intervals, not a kernel trace: the gaps between the graph's kernel nodes are inside.
frame   the ResNet-101 LiDAR detector (2 classes, seeded weights) on a 400 x 350 x 15 BEV blob at scale 0.5 as a captured
        frame (``model/frame_graph.FrameRunner``, filter included), one runner per setting, one stream; a window is
        ``--frames`` replays between two device events, windows alternate between the settings.  The count of boxes
        above the score threshold is reported with it: the pair work of the rotated rule grows with its square.

    python tools/rotated_nms_bench.py [--out profiles/rotated_nms.md]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

RROIS, SCORE_THRESH, MAX_DETS = 300, 0.1, 100


def prediction_set(n, k, seed):
    rng = np.random.default_rng(seed)
    cols = []
    for _ in range(k):
        m = (n + 2) // 3
        cars = np.stack((rng.uniform(0, 30, m), rng.uniform(0, 20, m), rng.uniform(-1, 1, m), rng.uniform(3, 5.5, m),
                         rng.uniform(1.5, 2.4, m), rng.uniform(1.4, 2.0, m), rng.uniform(-np.pi, np.pi, m)), 1)
        rows = cars[rng.integers(0, m, n)]
        rows[:, 0:2] += rng.normal(0, 0.15, (n, 2))
        rows[:, 3:6] *= 1 + rng.normal(0, 0.03, (n, 3))
        rows[:, 6] += rng.normal(0, 0.05, n)
        swap = rng.random(n) < 1 / 3
        rows[swap, 3], rows[swap, 4] = rows[swap, 4], rows[swap, 3]
        rows[swap, 6] += np.pi / 2
        cols.append(rows)
    return (np.ascontiguousarray(np.concatenate(cols, 1), dtype=np.float32),
            np.ascontiguousarray(rng.uniform(0, 1, (n, k)), dtype=np.float32))


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
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    assert torch.cuda.is_available(), "rotated_nms_bench needs the MI355X"
    dev = "cuda:0"
    C.reset_cfg()
    cfg = C.cfg
    nms_thresh = float(cfg.TEST.NMS_THRESH)

    def timed_replay(graph, units):
        def window():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3 / units
        return window

    lines = ["# Rotated BEV NMS (`cfg.TEST.NMS_ROTATED`) against the yaw-less LiDAR filter (`tools/rotated_nms_bench.py`)", "",
             "Command: `python tools/rotated_nms_bench.py --out profiles/rotated_nms.md` (reps %d, warm-up %d, %d calls per "
             "filter window, %d frames per frame window)." % (args.reps, args.warmup, args.inner, args.frames), "",
             "## The per-class filter, %d RoIs" % RROIS, "",
             "Device-event interval of one hipGraph replay holding %d back-to-back calls, per call; median (minimum) of %d "
             "windows, the two rules alternating.  Dense seeded prediction set (see the tool), score threshold %g, NMS "
             "threshold %g, max_dets %d." % (args.inner, args.reps, SCORE_THRESH, nms_thresh, MAX_DETS), "",
             "| classes | boxes above the score threshold per class | yaw-less us | rotated us | ratio | kept per class yaw-less | kept per class rotated |",
             "|---|---|---|---|---|---|---|"]
    for k in (2, 4):
        pb, cp = prediction_set(RROIS, k, 11 + k)
        pbd, cpd = torch.from_numpy(pb).to(dev), torch.from_numpy(cp).to(dev)
        cnt = torch.tensor([RROIS], dtype=torch.int32, device=dev)
        graphs, kept = {}, {}
        for rotated in (False, True):
            call = lambda: ops.filter_per_class_lidar(pbd, cpd, SCORE_THRESH, nms_thresh, 0, RROIS, roi_count=cnt,
                                                      rotated=rotated)
            kept[rotated] = call()[1].cpu().tolist()[1:]          # warm-up (LDS attributes) and the kept counts (no cut)
            call = lambda: ops.filter_per_class_lidar(pbd, cpd, SCORE_THRESH, nms_thresh, MAX_DETS, RROIS, roi_count=cnt,
                                                      rotated=rotated)
            call()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(args.inner):
                    call()
            graphs[rotated] = g
        t = alternate({r: timed_replay(g, args.inner) for r, g in graphs.items()}, args.reps, args.warmup)
        above = [(cp[:, c] > SCORE_THRESH).sum() for c in range(1, k)]
        med = {r: float(np.median(v)) for r, v in t.items()}
        lines.append("| %d | %s | %.1f (%.1f) | %.1f (%.1f) | %.1f | %s | %s |"
                     % (k, ", ".join(str(int(a)) for a in above), med[False] * 1e6, min(t[False]) * 1e6, med[True] * 1e6,
                        min(t[True]) * 1e6, med[True] / med[False], kept[False], kept[True]))
    frame_rot_us = None
    if not args.no_frame:
        from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
        from faster_rcnn_pytorch_multimodal_amd.nets.lidarnet import lidarnet
        from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
        cfg.NET_TYPE = "lidar"
        net = lidarnet(num_layers=101)
        net.create_architecture(2, tag="default", anchor_scales=cfg.LIDAR.ANCHOR_SCALES[0], anchor_ratios=cfg.LIDAR.ANCHOR_ANGLES)
        net.load_state_dict(seeded_state_dict(net, 9, bn_mode="tame"), strict=True)
        net.eval()
        net._device = dev
        net.to(dev)
        h, w = 400, 350
        rng = np.random.default_rng(3)
        blob = torch.from_numpy((rng.random((1, h, w, 15)) * (rng.random((1, h, w, 15)) < 0.05)).astype(np.float32)).to(dev)
        info = np.array([0, w, 0, h, 0, 12, 0.5], np.float32)
        runners, counts = {}, {}
        for rotated in (False, True):
            cfg.TEST.NMS_ROTATED = rotated
            runners[rotated] = FrameRunner(net, h, w, 15, info, thresh=SCORE_THRESH, max_dets=MAX_DETS, max_out=RROIS,
                                           autotune=not runners)
            dets, cnt = runners[rotated].run(blob)
            torch.cuda.synchronize()
            p = runners[rotated].predictions
            n = int(p["rois_count"].item())
            counts[rotated] = (n, int((p["cls_prob"][:n, 1] > SCORE_THRESH).sum().item()), cnt.cpu().tolist())

        def frame_window(r):
            def window():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.frames):
                    r.run(blob)
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e-3 / args.frames
            return window
        t = alternate({r: frame_window(x) for r, x in runners.items()}, args.reps, args.warmup)
        med = {r: float(np.median(v)) for r, v in t.items()}
        frame_rot_us = (med[True] - med[False]) * 1e6
        lines += ["", "## A LiDAR frame, %d x %d x 15 at scale 0.5, 2 classes, seeded weights" % (h, w), "",
                  "One captured frame per setting (filter included), one stream; device-event interval of %d replays, per "
                  "frame; median (minimum) of %d windows, the settings alternating.  %d RoIs, %d above the score threshold "
                  "%g." % (args.frames, args.reps, counts[True][0], counts[True][1], SCORE_THRESH), "",
                  "| `cfg.TEST.NMS_ROTATED` | ms per frame | frames/s | detections per class |", "|---|---|---|---|"]
        for r in (False, True):
            lines.append("| %s | %.3f (%.3f) | %.1f | %s |" % ("on" if r else "off", med[r] * 1e3, min(t[r]) * 1e3, 1 / med[r],
                                                           counts[r][2]))
        lines += ["", "Difference of the medians: %.1f us per frame = %.2f %% of the frame with the switch off."
                  % (frame_rot_us, 100 * (med[True] - med[False]) / med[False])]
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
