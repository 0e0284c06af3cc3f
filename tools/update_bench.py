#!/usr/bin/env python
"""Time of the weight update that ends a pseudo batch (``Network.apply_update``): the existing path (one clamp per
parameter, ``torch.optim.SGD`` with one param group per parameter, the bucket cleared) against ``cfg.TRAIN.FUSED_UPDATE``
(``model/train_val.FusedSGD``: one launch of ``frcnn_sgd_update`` over the gradient bucket), same process, same device.

The parameter list is the ResNet-101 + FPN image detector's (shapes from ``create_architecture``, seeded initialisation),
the gradients are random normals.  Both optimizers are built by ``SolverWrapper.construct_graph`` with the switch off and
on.  Per path:
    wall    ``--reps`` updates, each between two ``torch.cuda.synchronize()``, gradients refilled outside the timed
            region, after ``--warmup`` updates; the two paths alternate in blocks of ``--block`` updates; median and
            minimum.  This is what a training loop waits for: host work (Python loops, launches, the checks of
            FusedSGD) and device work.
    launch  (fused only) device-event interval around ``--inner`` back-to-back ``ops.sgd_update`` calls, median over
            ``--reps`` windows: the launch with its enqueue, without FusedSGD's per-parameter host work.  It is not a
            kernel trace: the achieved HBM rate derived from it (6 streams of 4 bytes per element: gradient read and
            cleared, momentum read and written, parameter read and written) is a lower bound of the kernel's.
The launches of the existing path are COUNTED from its operations (clamp_, the weight-decay add where wd != 0, the momentum
multiply and add, the parameter add: one launch each per parameter, as torch's multi-tensor path cannot batch across
single-parameter groups; plus the bucket's clear), not traced.

    python tools/update_bench.py [--out profiles/fused_update.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12            # bytes/s, MI355X specification
STEP_MS = 8.8                # README: one captured training step with four in flight
BATCH = 16                   # frames of a pseudo batch (cfg.TRAIN.BATCH_SIZE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--block", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import train_val
    from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
    assert torch.cuda.is_available(), "update_bench needs the MI355X"
    C.reset_cfg()
    cfg = C.cfg
    cfg.NET_TYPE = "image"
    cfg.USE_FPN = True
    cfg.POOLING_MODE = "multiscale"
    cfg.ENABLE_CUSTOM_TAIL = True
    torch.manual_seed(cfg.RNG_SEED)
    net = imagenet(num_layers=101)
    net.create_architecture(2, tag="default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    net._device = "cuda:0"
    net.to(net._device)
    net.train()

    def bind(bucket):
        """Both paths keep a gradient bucket of their own over the one net: make ``bucket``'s views the gradients."""
        off = 0
        for p in bucket.params:
            p.grad = bucket.flat[off:off + p.numel()].view_as(p)
            off += p.numel()

    def wall(optimizer, bucket, count, skip):
        bind(bucket)
        times = []
        for i in range(skip + count):
            bucket.flat.normal_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net.apply_update(optimizer, in_place=False)
            torch.cuda.synchronize()
            if i >= skip:
                times.append(time.perf_counter() - t0)
        return times

    solvers = {}
    for fused in (False, True):
        cfg.TRAIN.FUSED_UPDATE = fused
        solvers[fused] = train_val.SolverWrapper(net, 2, frames=None, log=lambda *_: None)
        solvers[fused].construct_graph()
        assert isinstance(solvers[fused].optimizer.optimizer, train_val.FusedSGD) == fused
    # the two paths ALTERNATE in blocks of --block updates (clocks, other tenants and allocator state drift over a run: a
    # path measured once after the other would carry that drift); the first block of each path also holds the warm-up
    times = {False: [], True: []}
    rounds = max(1, -(-args.reps // args.block))
    for r in range(rounds):
        for fused in (False, True):
            times[fused] += wall(solvers[fused].optimizer, solvers[fused].bucket, args.block, args.warmup if r == 0 else 1)
    results = {k: (float(np.median(v)), float(min(v))) for k, v in times.items()}
    groups = solvers[False].optimizer.param_groups
    launches = sum(4 + (1 if g["weight_decay"] != 0 else 0) for g in groups) + 1
    n_params, elems = len(groups), sum(p.numel() for g in groups for p in g["params"])
    # enqueue-inclusive device interval of the launch alone: ops.sgd_update directly (one ctypes call, the host-side table
    # check of the entry point, one launch), none of FusedSGD's per-parameter Python
    opt = solvers[True].optimizer.optimizer
    bind(solvers[True].bucket)
    call = lambda: ops.sgd_update(opt.bucket.flat, opt.momentum_flat, opt._seg_host, opt._seg_dev, opt._chunks_dev,
                                  opt.momentum, clip=float(cfg.GRAD_MAX_CLIP), zero_grads=True)
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    device = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            call()
        b.record()
        b.synchronize()
        device.append(a.elapsed_time(b) * 1e-3 / args.inner)
    t_dev, t_dev_min = float(np.median(device)), float(min(device))
    clip_v, mom_v = float(cfg.GRAD_MAX_CLIP), float(cfg.TRAIN.MOMENTUM)
    C.reset_cfg()
    (t_old, t_old_min), (t_new, t_new_min) = results[False], results[True]
    fused_launches = 2                                   # the update kernel and the clear of the bucket's fault slot
    rate = 6 * 4 * elems / t_dev
    batch_ms = BATCH * STEP_MS
    lines = [
        "# The weight update that ends a pseudo batch: `torch.optim.SGD` path against `cfg.TRAIN.FUSED_UPDATE` (`tools/update_bench.py`)",
        "",
        "ResNet-101 + FPN image detector: %d trainable parameters (one param group each), %d elements (%.1f MB of fp32 gradients); "
        "random gradients, clip %g, momentum %g.  Wall times: median (minimum) of %d updates between two device "
        "synchronisations, after %d warm-up updates.  Both paths in one process on one net, built by `SolverWrapper.construct_graph` "
        "with `cfg.TRAIN.FUSED_UPDATE` off and on, alternating in blocks of %d updates."
        % (n_params, elems, elems * 4 / 1e6, clip_v, mom_v, len(times[False]), args.warmup, args.block),
        "",
        "| path | wall ms per update | launches per update | share of a %d-frame pseudo batch at %.1f ms per step |" % (BATCH, STEP_MS),
        "|---|---|---|---|",
        "| existing (clamp per parameter, `torch.optim.SGD`, clear) | %.3f (%.3f) | %d (counted from the operations, not traced) | %.2f %% |"
        % (t_old * 1e3, t_old_min * 1e3, launches, 100 * t_old * 1e3 / (batch_ms + t_old * 1e3)),
        "| fused (`FusedSGD.fused_update`) | %.3f (%.3f) | %d | %.2f %% |"
        % (t_new * 1e3, t_new_min * 1e3, fused_launches, 100 * t_new * 1e3 / (batch_ms + t_new * 1e3)),
        "",
        "Launches removed: %d.  Wall time ratio existing / fused: %.1f." % (launches - fused_launches, t_old / t_new),
        "",
        "Device interval of the launch alone, enqueue included (device events around %d back-to-back `ops.sgd_update` calls - one "
        "ctypes call and one launch each, none of `FusedSGD`'s per-parameter Python - median (minimum) of %d windows; NOT a kernel "
        "trace, so host enqueue time between launches is inside it and the rate is a lower bound of the kernel's): %.1f (%.1f) us "
        "per update = %.2f TB/s over 6 streams x 4 bytes x %d elements = %.0f %% of the %.1f TB/s HBM peak (specification)."
        % (args.inner, args.reps, t_dev * 1e6, t_dev_min * 1e6, rate / 1e12, elems, 100 * rate / HBM_PEAK, HBM_PEAK / 1e12),
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
