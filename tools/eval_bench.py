#!/usr/bin/env python
"""Scoring time of a detections file: the host path of ``waymo_eval`` against its ``device='cuda'`` branch
(``frcnn_eval_match``), for the rotated types 'bev' and '3d'.

Scene: ``--frames`` x ``--dets`` detections x ``--gt`` gt boxes per frame (default 200 x 50 x 20 = 2e5 pairs).  Per type:
    host        waymo_eval(...) as it is without ``device``           one run, wall clock
    whole call  waymo_eval(..., device='cuda')                        median of ``--reps`` runs, wall clock; the call ends
                                                                      in device-to-host copies, so the device is idle after
    launch      ops.eval_match on tensors already on the device       median of ``--reps`` device-event intervals, each
                                                                      around ``--inner`` launches, after a warm-up
The results of the two paths are compared (tables equal, AP within 1e-12) before any time is printed.

    python tools/eval_bench.py [--out profiles/device_eval.md]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def make_scene(frames, dets, gt, seed=0):
    from faster_rcnn_pytorch_multimodal_amd.datasets.waymo_eval import make_rec
    rng = np.random.default_rng(seed)

    def boxes(n):
        return np.column_stack((rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-1, 1, n), rng.uniform(3, 5, n),
                                rng.uniform(1.5, 2.5, n), rng.uniform(1.4, 2.0, n), rng.uniform(-np.pi, np.pi, n)))

    recs, tokens, conf, out = [], [], [], []
    for f in range(frames):
        g = boxes(gt)
        d = g[rng.integers(0, gt, dets)].copy()
        d[:, :3] += rng.normal(0, 0.3, (dets, 3))
        d[:, 3:6] *= rng.uniform(0.9, 1.1, (dets, 3))
        d[:, 6] += rng.normal(0, 0.1, dets)
        d[dets * 4 // 5:] = boxes(dets - dets * 4 // 5)
        name = "%06d.bin" % f
        recs.append(make_rec(name, g, difficulty=rng.integers(1, 4, gt), ignore=rng.random(gt) < 0.1, boxes_dc=boxes(2)))
        tokens += [name] * dets
        conf += list(rng.uniform(0.05, 1, dets))
        out.append(d)
    return recs, tokens, np.array(conf), np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--dets", type=int, default=50)
    ap.add_argument("--gt", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.datasets import device_eval as D
    from faster_rcnn_pytorch_multimodal_amd.datasets.waymo_eval import waymo_eval
    assert torch.cuda.is_available(), "eval_bench needs the MI355X"
    recs, tokens, conf, boxes = make_scene(args.frames, args.dets, args.gt)
    pairs = args.frames * args.dets * (args.gt + 2)
    path = os.path.join(tempfile.mkdtemp(), "det.txt")
    with open(path, "w") as fh:
        for i, (t, c, b) in enumerate(zip(tokens, conf, boxes)):
            fh.write("%d %s %r %s\n" % (i, t, float(c), " ".join(repr(float(v)) for v in b)))
    lines = ["# Scoring a detections file: host loop against `frcnn_eval_match` (`tools/eval_bench.py`)", "",
             "%d frames x %d detections x (%d gt + 2 don't-care) boxes = %d pairs, ovthresh 0.7, don't-care boxes consulted."
             % (args.frames, args.dets, args.gt, pairs), "",
             "| type | host s | whole call ms (median, min) | launch us (median, min) | host pairs/s | whole-call pairs/s | "
             "launch pairs/s | upload + launch + read-back ms | host CSR build ms |", "|---|---|---|---|---|---|---|---|---|"]
    for eval_type in ("bev", "3d"):
        t0 = time.perf_counter()
        host = waymo_eval(path, recs, 0.7, eval_type, 2, bbox_elem=7, ignore_dc=True)[3]
        t_host = time.perf_counter() - t0
        dev = waymo_eval(path, recs, 0.7, eval_type, 2, bbox_elem=7, ignore_dc=True, device="cuda")[3]      # warm-up
        for key in ("tp", "fp", "npos"):
            assert np.array_equal(host[key], dev[key]), key
        assert np.abs(host["ap"] - dev["ap"]).max() <= 1e-12
        whole = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            waymo_eval(path, recs, 0.7, eval_type, 2, bbox_elem=7, ignore_dc=True, device="cuda")
            whole.append(time.perf_counter() - t0)
        prep, match = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            p = D.prepare(tokens, conf, boxes, recs, eval_type, True)
            prep.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            D.match(tokens, conf, boxes, recs, 0.7, eval_type, True)
            match.append(time.perf_counter() - t0)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).cuda()

        dev_args = [up(p.det_boxes), up(p.det_rows), up(p.det_offsets), up(p.gt_boxes), up(p.gt_ignore), up(p.gt_difficulty),
                    up(p.gt_offsets), eval_type, 0.7, 0.5, up(p.dc_boxes), up(p.dc_offsets)]
        for _ in range(5):
            ops.eval_match(*dev_args, max_gt_per_frame=p.max_gt_per_frame)
        torch.cuda.synchronize()
        launch = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                ops.eval_match(*dev_args, max_gt_per_frame=p.max_gt_per_frame)
            b.record()
            b.synchronize()
            launch.append(a.elapsed_time(b) * 1e-3 / args.inner)
        w, l = float(np.median(whole)), float(np.median(launch))
        lines.append("| %s | %.2f | %.1f, %.1f | %.0f, %.0f | %.3g | %.3g | %.3g | %.1f | %.1f |"
                     % (eval_type, t_host, w * 1e3, min(whole) * 1e3, l * 1e6, min(launch) * 1e6, pairs / t_host, pairs / w,
                        pairs / l, (float(np.median(match)) - float(np.median(prep))) * 1e3, float(np.median(prep)) * 1e3))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
