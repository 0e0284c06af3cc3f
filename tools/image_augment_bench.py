#!/usr/bin/env python
"""Image augmentation timing: every stage of ``frcnn_image_augment`` alone on a 1280 x 1920 x 3 uint8 frame, the worst-case
record (flip + Gaussian 9 taps + noise + bilinear affine + per-channel dropout) and the expected draw mix, each next to
``frcnn_prep_image`` on the same frame at scale 1.0 (the pass over the same pixels that exists without the augmentation).
HIP events around ``--inner`` back-to-back calls, warm-up first, ``--reps`` repetitions, median and 10th - 90th percentile
of the per-call time.  Bytes moved = one read and one write of H*W*3 per stage (prep: H*W*3 read, H*W*3*4 written).
Writes a markdown report.

    python tools/image_augment_bench.py [--reps 30] [--inner 20] [--out profiles/image_augment.md]
    python tools/image_augment_bench.py --trace-loop 20       # bare launch loop to put under a kernel trace
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_MEASURED_TBS = 6.29          # float4 copy on an MI355X


def frame(h, w, seed=0):
    rng = np.random.default_rng(seed)
    im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    im[: h // 4, : w // 3] = (90, 140, 30)
    im[h // 2:, w // 2:] = (im[h // 2:, w // 2:] // 4) + 96
    return np.ascontiguousarray(im)


def time_us(fn, reps, inner, warmup=5):
    for _ in range(warmup * inner):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(1e3 * e0.elapsed_time(e1) / inner)
    return float(np.median(times)), float(np.percentile(times, 10)), float(np.percentile(times, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--mix", type=int, default=400, help="records drawn for the expected draw mix")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-loop", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.image_augment import Affine, ImageAugment, draw_image_augmentation
    from faster_rcnn_pytorch_multimodal_amd.utils.blob import prep_im_for_blob
    C.reset_cfg()
    h, w = args.height, args.width
    img = torch.from_numpy(frame(h, w)).to("cuda:0")
    out = torch.empty_like(img)
    scratch = torch.empty(_hip.load().frcnn_image_augment_ws_bytes(h, w), dtype=torch.uint8, device="cuda:0")
    aff = dict(scale_x=1.1, scale_y=0.95, translate_x=0.03, translate_y=-0.02, shear=0.05, cval=17)
    worst = ImageAugment(flip=True, stages=(('gaussian', 2.5), ('noise', 12.0)), affine=Affine(order=1, **aff),
                         dropout=(0.04, True), seed=1)
    records = [
        ("flip alone", ImageAugment(flip=True)),
        ("Gaussian 5 taps", ImageAugment(stages=(('gaussian', 1.0),))),
        ("Gaussian 7 taps", ImageAugment(stages=(('gaussian', 2.0),))),
        ("Gaussian 9 taps", ImageAugment(stages=(('gaussian', 2.5),))),
        ("average 2x2", ImageAugment(stages=(('average', 2),))),
        ("average 3x3", ImageAugment(stages=(('average', 3),))),
        ("median 3x3", ImageAugment(stages=(('median', 3),))),
        ("sharpen", ImageAugment(stages=(('sharpen', 0.6, 1.2),))),
        ("noise", ImageAugment(stages=(('noise', 12.0),), seed=1)),
        ("hue / saturation", ImageAugment(stages=(('hue_sat', 5, -4),))),
        ("affine nearest", ImageAugment(affine=Affine(order=0, **aff))),
        ("affine bilinear", ImageAugment(affine=Affine(order=1, **aff))),
        ("dropout, one mask", ImageAugment(dropout=(0.04, False), seed=1)),
        ("dropout per channel", ImageAugment(dropout=(0.04, True), seed=1)),
        ("worst case (flip + Gaussian 9 + noise + affine bilinear + dropout per channel)", worst),
    ]

    def prep():
        prep_im_for_blob(img, im_scale=1.0, device="cuda:0")

    if args.trace_loop:
        for _ in range(args.trace_loop):
            prep()
            for _, aug in records:
                ops.image_augment(img, aug, out=out, scratch=scratch)
        torch.cuda.synchronize()
        return
    frame_bytes = h * w * 3
    p, p10, p90 = time_us(prep, args.reps, args.inner)
    lines = ["# `frcnn_image_augment` next to `frcnn_prep_image` (`tools/image_augment_bench.py`)", "",
             "%d x %d x 3 uint8 frame (%.1f MB).  HIP events around %d back-to-back calls, %d repetitions after warm-up; median"
             % (h, w, frame_bytes / 1e6, args.inner, args.reps),
             "(10th - 90th percentile) per call in microseconds.  Bytes = one read + one write of the frame per stage; the frame",
             "is smaller than the 256 MiB Infinity Cache, so the bytes/s column is a rate against the measured HBM copy rate of",
             "%.2f TB/s, not a claim that the bytes came from HBM." % HBM_MEASURED_TBS, "",
             "`frcnn_prep_image` at scale 1.0 (reads %.1f MB, writes %.1f MB): **%.1f us** (%.1f - %.1f)."
             % (frame_bytes / 1e6, 4 * frame_bytes / 1e6, p, p10, p90), "",
             "| record | launches | us per call | x prep | GB/s | of %.2f TB/s |" % HBM_MEASURED_TBS,
             "|---|---:|---:|---:|---:|---:|"]
    for name, aug in records:
        n = max(len(ops.image_augment_stages(aug, h, w)[1]), 1)
        t, t10, t90 = time_us(lambda: ops.image_augment(img, aug, out=out, scratch=scratch), args.reps, args.inner)
        gbs = 2.0 * frame_bytes * n / (t * 1e-6) / 1e9
        lines.append("| %s | %d | %.1f (%.1f - %.1f) | %.2f | %.0f | %.1f %% |"
                     % (name, n, t, t10, t90, t / p, gbs, 100.0 * gbs / (HBM_MEASURED_TBS * 1e3)))
    # the expected draw mix: records drawn like the data layer draws them, identity ones cost nothing
    rng = np.random.default_rng(0)
    mix = [draw_image_augmentation(w, h, rng) for _ in range(args.mix)]
    active = [a for a in mix if not a.identity]

    def run_mix():
        for a in active:
            ops.image_augment(img, a, out=out, scratch=scratch)

    m, m10, m90 = time_us(run_mix, max(args.reps // 6, 3), 1, warmup=1)
    launches = sum(max(len(ops.image_augment_stages(a, h, w)[1]), 1) for a in active)
    lines += ["", "Expected draw mix (%d records from `draw_image_augmentation`, %d of them the identity and free, %.2f launches per"
              % (len(mix), len(mix) - len(active), launches / len(mix)),
              "frame on average): **%.1f us per frame** (%.1f - %.1f), %.2f x `frcnn_prep_image`; host time of the Python wrapper"
              % (m / len(mix), m10 / len(mix), m90 / len(mix), m / len(mix) / p),
              "included when it exceeds the kernels'."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
