#!/usr/bin/env python
"""What drawing the detections costs (model/draw.py, csrc/draw.hip).

    render   device time of ``render_frame`` - every launch of one frame's picture (canvas, plan, clear, scatter, compose; three
             more for the BEV extrema) - device events around ``--inner`` calls on one stream, median of ``--reps``, after a
             warm-up: a 1000 x 600 camera frame with 100 and with 300 boxes, a 400 x 350 x 15 BEV frame with 100.
    png      host time of ``write_png`` for one such picture, one thread, median of ``--reps``.
    loop     frames/s of ``test_net`` over 18 distinct 1000 x 600 frames (the drop-in test's loop: res101, graphs replayed,
             four frames in flight) with ``draw_det`` off and on, in one process, alternating, ``--passes`` passes each after
             a warm-up pass of each; wall clock from the first frame queued to the last record on the host and the last
             picture on disk (``timers['loop_s']``).  With ``draw_det`` off nothing of the drawing is allocated or launched:
             that figure is the loop's rate as it was before the drawing existed.

    python tools/draw_bench.py [--out profiles/draw_det.md]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def _record(rng, k, max_out, n, lidar, h, w):
    elem = 8 if lidar else 5
    dets = np.zeros((k, max_out, elem), np.float32)
    if lidar:
        dets[1, :, 0], dets[1, :, 1] = rng.uniform(0, w, max_out), rng.uniform(0, h, max_out)
        dets[1, :, 3:6] = rng.uniform(5, 40, (max_out, 3))
        dets[1, :, 6] = rng.uniform(-np.pi, np.pi, max_out)
    else:
        x0, y0 = rng.uniform(0, w - 60, max_out), rng.uniform(0, h - 60, max_out)
        dets[1, :, 0], dets[1, :, 1] = x0, y0
        dets[1, :, 2], dets[1, :, 3] = x0 + rng.uniform(20, 400, max_out), y0 + rng.uniform(20, 300, max_out)
    dets[1, :, elem - 1] = rng.uniform(0, 1, max_out)
    return dets, np.array([0, n], np.int32)


def time_render(torch, lidar, h, w, boxes, inner, reps):
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model.draw import render_frame
    C.reset_cfg()
    C.cfg.NET_TYPE = "lidar" if lidar else "image"
    rng = np.random.default_rng(boxes + h)
    if lidar:
        blob = (rng.random((1, h, w, 15)) * (rng.random((1, h, w, 15)) < 0.05)).astype(np.float32)
    else:
        blob = (rng.standard_normal((1, h, w, 3)) * 60).astype(np.float32)
    dets, counts = _record(rng, 2, 300, boxes, lidar, h, w)
    gt = np.array(dets[1, :8, :7 if lidar else 4])
    blob, dets, counts = (torch.from_numpy(a).to(DEV) for a in (blob, dets, counts))
    gt = (torch.from_numpy(gt).to(DEV), torch.ones(8, dtype=torch.int32, device=DEV))
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=DEV)
    scratch = {"owner": torch.empty((h, w), dtype=torch.int32, device=DEV),
               "ws": ops.canvas_bev_workspace(DEV) if lidar else None}
    info = np.array([0, w, 0, h, 0, 12 if lidar else 0, 1.0], np.float32)
    run = lambda: render_frame(blob, info, dets, counts, gt=gt, out=out, scratch=scratch)
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / inner)
    picture = out.cpu().numpy()
    C.reset_cfg()
    return statistics.median(times), min(times), max(times), picture


def time_png(picture, reps, folder):
    from faster_rcnn_pytorch_multimodal_amd.model.draw import write_png
    times = []
    path = os.path.join(folder, "png_probe.png")
    for _ in range(reps):
        t = time.perf_counter()
        write_png(path, picture)
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), os.path.getsize(path)


class Frames:
    num_classes = 2
    name = "draw_bench"

    def __init__(self, blobs, info):
        self.blobs, self.info = blobs, info

    def num_frames(self, mode):
        return len(self.blobs)

    def blobs_at(self, i, mode):
        return {"data": self.blobs[i], "info": self.info}

    def name_at(self, i, mode):
        return "frame_%02d" % i

    def gt_at(self, i, mode):
        return {"boxes": np.array([[100, 80, 400, 300], [500, 200, 900, 550]], np.float32), "gt_classes": np.array([1, 1], np.int32)}


def time_loop(torch, passes, folder):
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model.test import test_net
    from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
    from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
    C.reset_cfg()
    C.cfg.NET_TYPE = "image"
    C.cfg.ROOT_DIR = folder
    net = imagenet(num_layers=101)
    net.create_architecture(2, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
    net.load_state_dict(seeded_state_dict(net, 7, bn_mode="tame"))
    net.eval()
    net._device = DEV
    net.to(DEV)
    rng = np.random.default_rng(23)
    means = C.cfg.PIXEL_MEANS.reshape(1, 1, 1, 3)
    blobs = [torch.from_numpy((rng.integers(0, 256, (1, 600, 1000, 3)) - means).astype(np.float32)).to(DEV) for _ in range(18)]
    src = Frames(blobs, np.array([0, 1000, 0, 600, 0, 0, 1.0], np.float32))
    rates = {False: [], True: []}
    boxes = 0
    for p in range(passes + 1):
        for draw in (False, True):
            timers = {}
            all_boxes = test_net(net, src, os.path.join(folder, "eval"), max_dets=100, thresh=0.05, mode="val", draw_det=draw,
                                 timers=timers)
            if p:                                                        # pass 0 warms up (captures, autotune, pinned buffers)
                rates[draw].append(timers["frames"] / timers["loop_s"])
            boxes = sum(len(np.asarray(b).reshape(-1, 5)) for b in all_boxes[1]) / 18.0
    C.reset_cfg()
    return rates, boxes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("draw_bench: no GPU visible; these are device timings")
    folder = tempfile.mkdtemp(prefix="draw_bench_")
    lines = ["| what | median | min .. max |", "|---|---|---|"]
    try:
        pictures = {}
        for name, lidar, h, w, boxes in (("render, 1000 x 600 image, 100 boxes + 8 gt", False, 600, 1000, 100),
                                         ("render, 1000 x 600 image, 300 boxes + 8 gt", False, 600, 1000, 300),
                                         ("render, 400 x 350 x 15 BEV, 100 footprints + 8 gt", True, 400, 350, 100)):
            med, lo, hi, pictures[name] = time_render(torch, lidar, h, w, boxes, args.inner, args.reps)
            lines.append("| %s | %.1f us | %.1f .. %.1f us |" % (name, med, lo, hi))
        for name, pic in pictures.items():
            if "300" in name:
                continue
            med, size = time_png(pic, args.reps, folder)
            lines.append("| write_png of the %s picture, one thread | %.1f ms (%.2f MB file) | |"
                         % ("BEV" if "BEV" in name else "camera (noise)", med, size / 1e6))
        if not args.skip_loop:
            rates, boxes = time_loop(torch, args.passes, folder)
            for draw in (False, True):
                r = rates[draw]
                lines.append("| test_net, 18 frames 1000 x 600, draw_det=%s | %.1f frames/s | %.1f .. %.1f |"
                             % (draw, statistics.median(r), min(r), max(r)))
            lines.append("| on / off | %.2f | %.1f boxes drawn per frame |"
                         % (statistics.median(rates[True]) / statistics.median(rates[False]), boxes))
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
