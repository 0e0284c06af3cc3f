#!/usr/bin/env python
"""What the camera field-of-view step of KITTI / CADC scans costs in front of ``frcnn_bev_voxelize``: four legs on the same
cloud (HIP events, warm-up, median and 10th - 90th percentile over many repetitions, the legs alternating in one run):

    voxelise alone                               get_lidar_blob
    field of view + voxelise                     frcnn_lidar_augment_fov with every other step off
    field of view + training record + voxelise   frcnn_lidar_augment_fov with the record
    training record + voxelise                   frcnn_lidar_augment with the record: the path without the step

The fourth leg is the code path the library had before the step existed; the third against the fourth is what the step
adds to a training frame.  Writes a markdown report.

    python tools/lidar_fov_bench.py [--points 60000 120000 180000] [--reps 200] [--out profiles/lidar_fov.md]
    python tools/lidar_fov_bench.py --trace-loop 50        # bare launch loop to put under a kernel trace
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lidar_augment_bench import median_us  # noqa: E402


def cloud(n, seed=0):
    """A scan around the sensor (every octant), F = 4, a few dense voxels in front of the camera."""
    rng = np.random.default_rng(seed)
    pts = np.stack((rng.uniform(-30, 75, n), rng.uniform(-45, 45, n), rng.uniform(-3.3, 3.3, n), rng.uniform(0, 3, n)),
                   1).astype(np.float32)
    pts[:n // 20, :3] = rng.normal([14, 1, -1], [0.5, 0.5, 0.3], (n // 20, 3))
    return np.ascontiguousarray(pts[rng.permutation(n)])


def kitti_like_projection():
    """M = P2 . [R0 0; 0 1] . [Tr; 0 0 0 1] of a made-up KITTI-like calibration (velodyne x front, y left, z up)."""
    p2 = np.array([[721.5, 0, 609.6, 44.86], [0, 721.5, 172.9, 0.2164], [0, 0, 1, 0.002746]])
    tr = np.eye(4)
    tr[:3, :3] = [[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]
    tr[:3, 3] = [-0.004, -0.076, -0.272]
    return p2 @ tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[60000, 120000, 180000])
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
    proj, img_size = kitti_like_projection(), list(cfg.KITTI.IMG_SIZE)
    record = LidarAugment(flip_x=True, flip_y=True, swap_xy=True, gauss=(0.05, 0.05, 0.03), p_keep=0.9, seed=1)
    nothing = LidarAugment()
    lines = ["# The field-of-view step of `frcnn_lidar_augment_fov` next to `frcnn_bev_voxelize` (`tools/lidar_fov_bench.py`)", "",
             "HIP events around each call on an idle device, %d repetitions after 20 warm-up rounds, the legs alternating;"
             % args.reps,
             "median (10th - 90th percentile) in microseconds.  Scale %.2f (grid %d x %d), F = 4, KITTI-like camera (%d x %d)."
             % (args.scale, int(80 * 10 * args.scale), int(70 * 10 * args.scale), img_size[1], img_size[0]),
             "Training record: flips, swap, distortion, dropout.  `fov adds` = (fov + record + voxelise) - (record + voxelise).", "",
             "| points | inside the frame | voxelise alone | fov + voxelise | fov + record + voxelise | record + voxelise "
             "(the path without the step) | fov adds | fov adds / (record + voxelise) |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for n in args.points:
        pts = torch.from_numpy(cloud(n)).to("cuda:0")
        out = torch.empty_like(pts)

        def vox():
            get_lidar_blob(pts, args.scale, device="cuda:0")

        def fov_vox():
            moved, _ = ops.lidar_augment_points(pts, nothing, 0, extents, out=out, proj=proj, img_size=img_size)
            get_lidar_blob(moved, args.scale, device="cuda:0")

        def fov_record_vox():
            moved, _ = ops.lidar_augment_points(pts, record, record.seed, extents, out=out, proj=proj, img_size=img_size)
            get_lidar_blob(moved, args.scale, device="cuda:0")

        def record_vox():
            moved, _ = ops.lidar_augment_points(pts, record, record.seed, extents, out=out)
            get_lidar_blob(moved, args.scale, device="cuda:0")

        if args.trace_loop:
            for _ in range(args.trace_loop):
                fov_vox()
                fov_record_vox()
                record_vox()
            torch.cuda.synchronize()
            continue
        inside = int(ops.lidar_fov_filter(pts, proj, img_size)[1].item())
        (v, v10, v90), (f, f10, f90), (fr, fr10, fr90), (r, r10, r90) = median_us([vox, fov_vox, fov_record_vox, record_vox],
                                                                                  args.reps)
        lines.append("| %d | %d | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.1f | %.1f %% |"
                     % (n, inside, v, v10, v90, f, f10, f90, fr, fr10, fr90, r, r10, r90, fr - r, 100.0 * (fr - r) / r))
    if args.trace_loop:
        return
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
