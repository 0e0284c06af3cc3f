#!/usr/bin/env python
"""Cost of cfg.TRAIN.CONV_BF16 on the image detector's 1000 x 600 ResNet-101 + FPN training step (tools/bench_configs.py's
net, weights, frame and boxes: BASELINE.json configs[3]).  Same process, same device, switch off against switch on.

shapes  every distinct eligible convolution of one step, per family, as the step issues it (recorded from one eager step with
        the switch on): forward ``ops.conv2d_nhwc`` under the plans the step's own warm-up tuned (a Winograd plan gets its
        pre-transformed filter) against ``ops.conv2d_nhwc_bf16``; data gradient ``ops.conv2d_bwd_data`` (Winograd filter and
        the fused activation backward as the step uses them) against ``ops.conv2d_bwd_data_bf16``; filter gradient
        ``ops.conv2d_bwd_weight_acc`` (one layer at a time - the captured fp32 step launches repeated layers GROUPED, which this
        column does not show) against ``ops.conv2d_bwd_weight_acc_bf16``.  The strided 1x1 data gradient stays fp32 under the
        switch and is listed as such.  ``--inner`` back-to-back calls are captured into one hipGraph per form; a window is one
        replay between two device events; the forms alternate window by window, ``--reps`` windows each after ``--warmup``;
        median per call.  Random normal operands.
step    the whole step three ways - eager, captured (one chain, one frame at a time), four frames in flight
        (``TrainPipeline``) - as tools/bench_configs.py times them (8 untimed steps, median of 3 windows of ``--steps``
        steps, an SGD update every 16), every run from the same weights; off, on, off, on.

    python tools/conv_bf16_train_bench.py [--out profiles/conv_bf16_train.md]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from conv_bf16_bench import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench_configs as BC
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    assert torch.cuda.is_available(), "conv_bf16_train_bench needs the MI355X"
    dev = "cuda:0"
    net, opt, blobs = BC._build_fpn_train()
    cfg = C.cfg
    BC._tune_and_count(net, opt, blobs, True)           # the fp32 plans of every shape of the step
    start = BC._snapshot(net)

    # ---- the step's eligible convolutions, as issued ----------------------------------------------------------------------
    issued = {"fwd": {}, "dgrad": {}, "wgrad": {}}
    real = {n: getattr(ops, n) for n in ("conv2d_nhwc_bf16", "conv2d_bwd_data_bf16", "conv2d_bwd_data", "conv2d_bwd_weight_bf16")}

    def note(family, key):
        issued[family][key] = issued[family].get(key, 0) + 1

    def fwd(x, w_bf16, scale=None, shift=None, residual=None, stride=1, pad=0, relu=False, out=None):
        note("fwd", tuple(x.shape) + (w_bf16.shape[0], w_bf16.shape[1], stride, pad, residual is not None, bool(relu)))
        return real["conv2d_nhwc_bf16"](x, w_bf16, scale, shift, residual, stride=stride, pad=pad, relu=relu, out=out)

    def dgrad(dy, w_t_bf16, x_shape, stride=1, pad=0, add=None, act_y=None, act_scale=None, out=None, ws=None):
        note("dgrad", tuple(x_shape) + (w_t_bf16.shape[3], w_t_bf16.shape[1], stride, pad, add is not None, act_y is not None, True))
        return real["conv2d_bwd_data_bf16"](dy, w_t_bf16, x_shape, stride=stride, pad=pad, add=add, act_y=act_y, act_scale=act_scale)

    def dgrad_fp32(dy, w_t, x_shape, stride=1, pad=0, add=None, w_winograd=None, act_y=None, act_scale=None):
        # under the switch the only fp32 data gradients of eligible layers are the strided 1x1 ones
        if stride > 1 and w_t.shape[1] == 1 and w_t.shape[0] % 32 == 0 and w_t.shape[3] % 32 == 0:
            note("dgrad", tuple(x_shape) + (w_t.shape[3], 1, stride, pad, add is not None, act_y is not None, False))
        return real["conv2d_bwd_data"](dy, w_t, x_shape, stride=stride, pad=pad, add=add, w_winograd=w_winograd, act_y=act_y,
                                       act_scale=act_scale)

    def wgrad(x, dy, r, s, stride=1, pad=0, want_bias=False, splits=0, out=None, ws=None):
        note("wgrad", tuple(x.shape) + (dy.shape[-1], r, stride, pad, bool(want_bias)))
        return real["conv2d_bwd_weight_bf16"](x, dy, r, s, stride=stride, pad=pad, want_bias=want_bias, splits=splits)

    ops.conv2d_nhwc_bf16, ops.conv2d_bwd_data_bf16, ops.conv2d_bwd_data, ops.conv2d_bwd_weight_bf16 = fwd, dgrad, dgrad_fp32, wgrad
    cfg.TRAIN.CONV_BF16 = True
    try:
        opt.zero_grad()
        net.train_step(blobs, opt, update_weights=False)
        torch.cuda.synchronize()
    finally:
        cfg.TRAIN.CONV_BF16 = False
        for n, fn in real.items():
            setattr(ops, n, fn)
    opt.zero_grad()

    def timed_replay(graph, units):
        def window():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3 / units
        return window

    def time_forms(forms):
        graphs = {}
        for name, call in forms.items():
            call()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(args.inner):
                    call()
            graphs[name] = gr
        t = alternate({nm: timed_replay(gr, args.inner) for nm, gr in graphs.items()}, args.reps, args.warmup)
        return {nm: float(np.median(v)) for nm, v in t.items()}

    lines = ["# bf16-operand convolutions in the training step (`cfg.TRAIN.CONV_BF16`) against the fp32 step "
             "(`tools/conv_bf16_train_bench.py`)", "",
             "Command: `python tools/conv_bf16_train_bench.py --out profiles/conv_bf16_train.md` (reps %d, warm-up %d, %d calls per "
             "shape window, %d steps per step window)." % (args.reps, args.warmup, args.inner, args.steps), ""]
    g = torch.Generator().manual_seed(0)
    rnd = lambda *shape: torch.randn(shape, generator=g).to(dev)
    totals = {}
    if not args.no_shapes:
        lines += ["## The step's eligible convolutions, shape by shape", "",
                  "1000 x 600 frame, FIXED_BLOCKS = 1.  us per call (median), fp32 / bf16 > 1 means bf16 is faster.  Data gradients marked "
                  "`fp32` are the strided 1x1 ones, which stay fp32 under the switch (their time counts on both sides).", ""]
        for family, title in (("fwd", "Forward"), ("dgrad", "Data gradient"), ("wgrad", "Filter gradient")):
            lines += ["### %s" % title, "", "| n h w c k r stride | form | calls per step | fp32 us | bf16 us | fp32 / bf16 |", "|---|---|---|---|---|---|"]
            tot = {"fp32": 0.0, "bf16": 0.0}
            for key, calls in issued[family].items():
                n, h, w, c, k, r, stride, pad = key[:8]
                ho, wo = ops.conv_out_hw(h, w, r, r, stride, pad)
                x, wt = rnd(n, h, w, c), rnd(k, r, r, c) * (r * r * c) ** -0.5
                if family == "fwd":
                    has_res, relu = key[8:]
                    scale, shift, res = rnd(k), rnd(k), (rnd(n, ho, wo, k) if has_res else None)
                    y = torch.empty((n, ho, wo, k), device=dev)
                    u = ops.winograd_filter(wt) if (not has_res and ops.winograd_filter_wanted(n, h, w, c, k, r, r, stride, pad)) else None
                    wp = ops.conv2d_pack_bf16(wt)
                    med = time_forms({"fp32": lambda: ops.conv2d_nhwc(x, wt, scale, shift, res, stride=stride, pad=pad, relu=relu, out=y, w_winograd=u),
                                      "bf16": lambda: ops.conv2d_nhwc_bf16(x, wp, scale, shift, res, stride=stride, pad=pad, relu=relu, out=y)})
                    form = ("residual " if has_res else "") + ("relu" if relu else "") + (" W" if u is not None else "")
                elif family == "dgrad":
                    has_add, has_act, is_bf16 = key[8:]
                    dy, w_t = rnd(n, ho, wo, k), ops.conv2d_transpose_filter(wt)
                    add = rnd(n, h, w, c) if has_add else None
                    act_y, act_scale = (rnd(n, h, w, c), rnd(c)) if has_act else (None, None)
                    u = ops.winograd_filter(w_t) if (not has_add and ops.dgrad_winograd_wanted((n, h, w, c), k, r, r, stride, pad)) else None
                    fp32 = lambda: ops.conv2d_bwd_data(dy, w_t, (n, h, w, c), stride=stride, pad=pad, add=add, w_winograd=u, act_y=act_y, act_scale=act_scale)
                    forms = {"fp32": fp32}
                    if is_bf16:
                        wp = ops.conv2d_pack_bf16(w_t)
                        forms["bf16"] = lambda: ops.conv2d_bwd_data_bf16(dy, wp, (n, h, w, c), stride=stride, pad=pad, add=add, act_y=act_y, act_scale=act_scale)
                    med = time_forms(forms)
                    med.setdefault("bf16", med["fp32"])
                    form = ("add " if has_add else "") + ("act " if has_act else "") + ("W " if u is not None else "") + ("" if is_bf16 else "fp32")
                else:
                    want_bias = key[8]
                    dy = rnd(n, ho, wo, k)
                    gw, gb = torch.zeros((k, c, r, r), device=dev), (torch.zeros(k, device=dev) if want_bias else None)
                    med = time_forms({"fp32": lambda: ops.conv2d_bwd_weight_acc(x, dy, r, r, gw, gb, stride=stride, pad=pad),
                                      "bf16": lambda: ops.conv2d_bwd_weight_acc_bf16(x, dy, r, r, gw, gb, stride=stride, pad=pad)})
                    form = "bias" if want_bias else ""
                tot["fp32"] += calls * med["fp32"]
                tot["bf16"] += calls * med["bf16"]
                lines.append("| %d %d %d %d %d %d %d | %s | %d | %.1f | %.1f | %.2f |"
                             % (n, h, w, c, k, r, stride, form.strip(), calls, med["fp32"] * 1e6, med["bf16"] * 1e6, med["fp32"] / med["bf16"]))
            totals[family] = tot
            lines += ["", "%s, sum over the step's calls (calls x median): fp32 %.3f ms, bf16 %.3f ms, ratio %.2f."
                      % (title, tot["fp32"] * 1e3, tot["bf16"] * 1e3, tot["fp32"] / tot["bf16"]), ""]
        lines += ["All three families: fp32 %.3f ms, bf16 %.3f ms, ratio %.2f." % (
            sum(t["fp32"] for t in totals.values()) * 1e3, sum(t["bf16"] for t in totals.values()) * 1e3,
            sum(t["fp32"] for t in totals.values()) / sum(t["bf16"] for t in totals.values())), ""]

    # ---- the whole step, three ways ---------------------------------------------------------------------------------------
    if not args.no_step:
        rows = []
        for mode in ("eager", "graph", "pipeline"):
            for rnd_i in range(2):
                for on in (False, True):
                    cfg.TRAIN.CONV_BF16 = on
                    BC._restore(net, opt, start)
                    net.enable_train_graphs(mode == "graph")
                    if mode == "pipeline":
                        losses, dt = BC._timed_pipeline_windows(net, blobs, opt, args.steps, 4)
                    else:
                        losses, dt = BC._timed_train_windows(net, blobs, opt, args.steps)
                    inline = ""
                    if mode == "graph":
                        inline = "one chain" if all(r.inline for r in net._train_graphs.values()) else "forked"
                    rows.append((mode, rnd_i, on, 1e3 * dt / args.steps, losses[0], losses[-1], inline))
                    net.enable_train_graphs(False)
        cfg.TRAIN.CONV_BF16 = False
        lines += ["## The 1000 x 600 ResNet-101 + FPN step", "",
                  "tools/bench_configs.py's windows (8 untimed steps, median of 3 windows of %d steps, SGD update every 16), every run "
                  "restored to the same weights; per way the settings alternate off, on, off, on." % args.steps, "",
                  "| way | run | `cfg.TRAIN.CONV_BF16` | ms per step | first loss | last loss | captured as |", "|---|---|---|---|---|---|---|"]
        for mode, rnd_i, on, ms, l0, l1, inline in rows:
            lines.append("| %s | %d | %s | %.2f | %.4f | %.4f | %s |" % (
                {"eager": "eager", "graph": "captured", "pipeline": "four in flight"}[mode], rnd_i + 1, "on" if on else "off", ms, l0, l1, inline))
        lines.append("")
        for mode in ("eager", "graph", "pipeline"):
            off = np.mean([r[3] for r in rows if r[0] == mode and not r[2]])
            on_ = np.mean([r[3] for r in rows if r[0] == mode and r[2]])
            lines.append("%s: off %.2f ms, on %.2f ms, off / on %.3f." % (mode, off, on_, off / on_))
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
