#!/usr/bin/env python
"""LiDAR input producer timing: ``frcnn_bev_voxelize`` alone against ``frcnn_lidar_augment`` + ``frcnn_bev_voxelize`` on the
same cloud (HIP events, warm-up, median over many repetitions, the two legs alternating in one run), the augment launch
alone and its achieved bytes/s (2 * N * F * 4 bytes moved once).  Writes a markdown report.

    python tools/lidar_augment_bench.py [--points 120000] [--reps 200] [--out profiles/lidar_augment.md]
    python tools/lidar_augment_bench.py --trace-loop 50        # bare launch loop to put under a kernel trace
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cloud(n, cols, seed=0):
    """A scan-like cloud: ~90 % of the points inside the 70 x 80 x 6 m range, a few dense voxels."""
    rng = np.random.default_rng(seed)
    pts = np.stack((rng.uniform(-2, 72, n), rng.uniform(-42, 42, n), rng.uniform(-3.2, 3.2, n), rng.uniform(0, 3, n),
                    rng.uniform(0, 2, n)), 1).astype(np.float32)
    pts[:n // 20, :3] = rng.normal([10, 0, -1], [0.5, 0.5, 0.3], (n // 20, 3))
    return np.ascontiguousarray(pts[rng.permutation(n)][:, :cols])


def median_us(legs, reps, warmup=20):
    """Median event-to-event time of each callable in ``legs``; the legs alternate inside every repetition and each
    starts on an idle device (a leg queued behind another one's kernels would hide its own launch latency), so a leg of a
    dozen short launches is timed as the data loader sees it: launch-bound."""
    for _ in range(warmup):
        for fn in legs:
            fn()
    times = [[] for _ in legs]
    for _ in range(reps):
        for t, fn in zip(times, legs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(1e3 * e0.elapsed_time(e1))
    return [(float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[90000, 180000])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-loop", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.lidar_augment import LidarAugment
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.minibatch import get_lidar_blob
    C.reset_cfg()
    C.cfg.NET_TYPE = "lidar"
    cfg = C.cfg
    extents = [cfg.LIDAR.X_RANGE[0], cfg.LIDAR.Y_RANGE[0], cfg.LIDAR.Z_RANGE[0],
               cfg.LIDAR.X_RANGE[1], cfg.LIDAR.Y_RANGE[1], cfg.LIDAR.Z_RANGE[1]]
    records = {
        "train (flips, swap, distortion, dropout)": LidarAugment(flip_x=True, flip_y=True, swap_xy=True,
                                                                 gauss=(0.05, 0.05, 0.03), p_keep=0.9, seed=1),
        "flips only": LidarAugment(flip_x=True, flip_y=True, seed=1),
        "test (rain 10 mm/h, dropout)": LidarAugment(rain_rate=10.0, rain_max_range=200.0, test_dropout=True, seed=1),
    }
    lines = ["# `frcnn_lidar_augment` next to `frcnn_bev_voxelize` (`tools/lidar_augment_bench.py`)", "",
             "HIP events around each call on an idle device, %d repetitions after 20 warm-up rounds, the legs alternating;"
             % args.reps,
             "median (10th - 90th percentile) in microseconds.  Scale %.2f (grid %d x %d).  `augment` moves 2 * N * F * 4 bytes."
             % (args.scale, int(80 * 10 * args.scale), int(70 * 10 * args.scale)), "",
             "| points x F | record | voxelise alone | augment + voxelise | added | added / voxelise | augment alone | GB/s |",
             "|---|---|---:|---:|---:|---:|---:|---:|"]
    for n in args.points:
        for cols in (4, 5):
            pts = torch.from_numpy(cloud(n, cols)).to("cuda:0")
            out = torch.empty_like(pts)
            elong = 4 if cols == 5 else None
            for name, aug in records.items():
                def vox():
                    get_lidar_blob(pts, args.scale, device="cuda:0", elongation=elong)

                def both():
                    moved, _ = ops.lidar_augment_points(pts, aug, aug.seed, extents, out=out)
                    get_lidar_blob(moved, args.scale, device="cuda:0", elongation=elong)

                def only():
                    ops.lidar_augment_points(pts, aug, aug.seed, extents, out=out)

                if args.trace_loop:
                    for _ in range(args.trace_loop):
                        both()
                    torch.cuda.synchronize()
                    continue
                (v, v10, v90), (b, b10, b90), (a, a10, a90) = median_us([vox, both, only], args.reps)
                gbs = 2.0 * n * cols * 4 / (a * 1e-6) / 1e9
                lines.append("| %d x %d | %s | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.1f | %.1f %% | %.1f (%.1f - %.1f) | %.0f |"
                             % (n, cols, name, v, v10, v90, b, b10, b90, b - v, 100.0 * (b - v) / v, a, a10, a90, gbs))
    if args.trace_loop:
        return
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
