#!/usr/bin/env python
"""Scoring time of a COCO results file: ``coco_eval.evaluate`` with ``device=None`` (plain loops, the yardstick) against
``device='cuda'`` (``frcnn_coco_match`` + the vectorised tail), split into prepare / matching / tail.

Scene (seeded): ``--images`` x ``--cats`` categories, about ``--gt`` ground-truth boxes and ``--dets`` detections per image
(default 5000 x 80, 7 and 100: the size of COCO val).  An image's boxes fall into a few categories; most detections are
jittered copies of a box of their image, the rest are strays in any category; 5 % of the boxes are crowd.

    device path  prepare    coco_eval.prepare: the CSR build on the host              wall clock, median of ``--reps``
                 match      upload, one launch, read back (coco_eval.match_device)    wall clock; ends in device-to-host copies
                 launch     ops.coco_match, boxes already on the device               device events around ``--inner`` calls,
                                                                                      median of ``--reps``, after a warm-up
                 tail       coco_eval.accumulate + compute_stats                      wall clock, median of ``--reps``
    host path    match_host and accumulate_loops on the FIRST ``--host-images`` images (0: all of them), one run each, wall
                 clock: the loops are the yardstick, not a product, and take minutes at full size.
The two paths are compared on the host subset (overlaps bit for bit, matches, precision, recall, scores and stats equal)
before any time is printed.

    python tools/coco_eval_bench.py [--out profiles/coco_eval.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def make_scene(images, cats, gt_per_image, dets_per_image, seed=0):
    """(GroundTruth, Results) built as flat arrays, in the order a dataset and a detector would write them."""
    from faster_rcnn_pytorch_multimodal_amd.datasets import coco_eval as C
    rng = np.random.default_rng(seed)
    n_gt = rng.poisson(gt_per_image, images)
    img_g = np.repeat(np.arange(images), n_gt)
    palette = rng.integers(0, cats, (images, 3))                 # an image's boxes fall into up to three categories
    cat_g = palette[img_g, rng.integers(0, 3, img_g.shape[0])]
    wh = np.exp(rng.uniform(np.log(8), np.log(300), (img_g.shape[0], 2)))
    xy = rng.uniform(0, 500, (img_g.shape[0], 2))
    bbox_g = np.round(np.concatenate([xy, wh], axis=1), 1)
    crowd = rng.random(img_g.shape[0]) < .05
    gt = C.GroundTruth(np.arange(images) * 7 + 1, np.arange(cats) + 1, img_g, cat_g, bbox_g,
                       bbox_g[:, 2] * bbox_g[:, 3] * rng.uniform(.5, 1, img_g.shape[0]), crowd)
    first = np.concatenate([[0], np.cumsum(n_gt)])
    img_d = np.repeat(np.arange(images), dets_per_image)
    n = img_d.shape[0]
    src = np.minimum(first[img_d] + (rng.random(n) * np.maximum(n_gt[img_d], 1)).astype(np.int64), max(img_g.shape[0] - 1, 0))
    stray = (rng.random(n) < .25) | (n_gt[img_d] == 0)
    jitter = rng.uniform(-.15, .15, (n, 4))
    box = bbox_g[src]
    box = np.concatenate([box[:, :2] + jitter[:, :2] * box[:, 2:], box[:, 2:] * (1 + jitter[:, 2:])], axis=1)
    cat_d = cat_g[src]
    k = int(stray.sum())
    box[stray] = np.concatenate([rng.uniform(0, 500, (k, 2)), np.exp(rng.uniform(np.log(8), np.log(300), (k, 2)))], axis=1)
    cat_d[stray] = rng.integers(0, cats, k)
    res = C.Results(gt.image_ids[img_d], gt.cat_ids[cat_d], box, np.round(rng.uniform(.05, 1, n), 3))
    return gt, res


def first_images(gt, res, count):
    from faster_rcnn_pytorch_multimodal_amd.datasets import coco_eval as C
    g, r = gt.img_index < count, res.image_id <= gt.image_ids[count - 1]
    return (C.GroundTruth(gt.image_ids[:count], gt.cat_ids, gt.img_index[g], gt.cat_index[g], gt.bbox[g], gt.area[g], gt.iscrowd[g]),
            C.Results(res.image_id[r], res.category_id[r], res.bbox[r], res.score[r]))


def clock(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times)), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--cats", type=int, default=80)
    ap.add_argument("--gt", type=float, default=7)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--host-images", type=int, default=250)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.datasets import coco_eval as C
    assert torch.cuda.is_available(), "coco_eval_bench needs the MI355X"
    params = C.Params()
    gt, res = make_scene(args.images, args.cats, args.gt, args.dets)
    host_images = args.images if args.host_images <= 0 else min(args.host_images, args.images)
    gt_h, res_h = first_images(gt, res, host_images)

    # the two paths on the host subset: equal before anything is timed
    p_h = C.prepare(gt_h, res_h, params)
    t0 = time.perf_counter()
    C.match_host(p_h, params)
    t_match_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_tables = C.accumulate_loops(p_h, params)
    t_acc_host = time.perf_counter() - t0
    dev_h = C.evaluate(gt_h, res_h, params, device="cuda")
    assert dev_h["ious"].tobytes() == p_h["ious"].tobytes()
    for key in ("dt_match", "dt_ignore", "gt_ignore"):
        assert np.array_equal(dev_h[key], p_h[key]), key
    for got, want in zip((dev_h["precision"], dev_h["recall"], dev_h["scores"]), host_tables):
        assert np.array_equal(got, want)
    assert np.array_equal(dev_h["stats"], C.compute_stats(host_tables[0], host_tables[1], params))

    # the device path at full size
    C.evaluate(gt, res, params, device="cuda")                                   # warm-up: code object, allocator
    p, prep_med, prep_min = clock(lambda: C.prepare(gt, res, params), args.reps)
    _, match_med, match_min = clock(lambda: C.match_device(p, params, "cuda"), args.reps)
    tables, tail_med, tail_min = clock(lambda: C.accumulate(p, params), args.reps)
    stats = C.compute_stats(tables[0], tables[1], params)
    _, whole_med, whole_min = clock(lambda: C.evaluate(gt, res, params, device="cuda"), args.reps)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    dev_args = (up(p["det"]), p["det_offsets"], up(p["gt"]), up(p["gt_crowd"]), p["gt_offsets"], up(params.iou_thrs),
                up(params.area_rng))
    for _ in range(3):
        ops.coco_match(*dev_args)
    torch.cuda.synchronize()
    launch = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            ops.coco_match(*dev_args)
        b.record()
        b.synchronize()
        launch.append(a.elapsed_time(b) * 1e-3 / args.inner)
    launch_med, launch_min = float(np.median(launch)), min(launch)

    n_pairs, n_det, n_gt = p["det_offsets"].shape[0] - 1, p["det"].shape[0], p["gt"].shape[0]
    cells = int(p["iou_offsets"][-1])
    walks = params.area_rng.shape[0] * params.iou_thrs.shape[0]
    out_bytes = cells * 8 + n_det * walks * 5 + n_gt * params.area_rng.shape[0]
    h_pairs, h_det, h_cells = p_h["det_offsets"].shape[0] - 1, p_h["det"].shape[0], int(p_h["iou_offsets"][-1])
    scale = cells / max(h_cells, 1)
    lines = [
        "# Scoring a COCO results file: host loops against `frcnn_coco_match` (`tools/coco_eval_bench.py`)", "",
        "Scene: %d images x %d categories, %d ground-truth boxes, %d detections in the file; %d (image, category) pairs, %d "
        "detections kept, %d overlaps, %d walks per pair.  AP %.4f, AP50 %.4f, AR@100 %.4f."
        % (args.images, args.cats, n_gt, len(res), n_pairs, n_det, cells, walks, stats[0], stats[1], stats[8]), "",
        "## Device path, full scene (median, min of %d)" % args.reps, "",
        "| step | time |", "|---|---|",
        "| prepare (host CSR build) | %.1f ms, %.1f ms |" % (prep_med * 1e3, prep_min * 1e3),
        "| match: upload, one launch, read back | %.1f ms, %.1f ms |" % (match_med * 1e3, match_min * 1e3),
        "| of which `ops.coco_match` alone (device events around %d calls; output allocations and the three offset uploads "
        "inside) | %.0f us, %.0f us |" % (args.inner, launch_med * 1e6, launch_min * 1e6),
        "| tail (vectorised accumulate + the 12 numbers) | %.1f ms, %.1f ms |" % (tail_med * 1e3, tail_min * 1e3),
        "| whole `evaluate(device='cuda')` | %.1f ms, %.1f ms |" % (whole_med * 1e3, whole_min * 1e3), "",
        "The launch writes %.1f MB of outputs (%.1f GB/s at the median) and makes %.3g walk steps over overlaps."
        % (out_bytes / 1e6, out_bytes / launch_med / 1e9, cells * walks), "",
        "## Host path, %s %d images (%d pairs, %d detections kept, %d overlaps), one run"
        % ("all" if host_images == args.images else "first", host_images, h_pairs, h_det, h_cells), "",
        "| step | time |", "|---|---|",
        "| `match_host` | %.2f s |" % t_match_host,
        "| `accumulate_loops` | %.2f s |" % t_acc_host, "",
        ("The host loops ran on the full scene." if host_images == args.images else
         "The full scene has %.1f x the overlaps of this subset; the host loops were not run on all of it (not measured)." % scale)
        + "  On the host path's images both paths were compared before timing: overlaps bit for bit, matches, ignore bytes, "
        "precision, recall, scores and the 12 numbers equal.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
