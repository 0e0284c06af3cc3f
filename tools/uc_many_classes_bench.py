#!/usr/bin/env python
"""The uncertainty heads at many classes: what the wide Bayesian cross entropy and the one-launch uncertainty columns cost.
Same process, same device; every time is taken inside a captured hipGraph (``--inner`` back-to-back calls per replay, one
replay between two device events, per call; median (minimum) of ``--calls`` replays, the sides alternating).

(a) bayes_ce   N = 256 RoIs, S = 200 samples: ``ops.bayesian_cross_entropy`` (one thread per RoI) at K = 2, 16 and
               ``ops.bayesian_cross_entropy_wide`` (one wave per RoI) at K = 16, 17, 21, 81, gradients included.
(b) columns    ``ops.uncertainty_columns`` against the torch statement it replaces (``stack_uncertainty_columns`` +
               ``torch.cat``: one gather per class and box-variance kind) at K = 2, 4, 21, 81; R = 300 RoIs, 100 rows per
               class, image boxes, all eight sources.
(c) frame      the captured 1000 x 600 ResNet-101 TEST frame with 21 classes and all four cfg.UC.EN_* flags, filter
               included: with the one-launch columns, and with the torch statement in their place (the previous path; nothing
               else in the frame differs between the two).
(d) untouched  ``ops.logit_distort`` + ``ops.mc_cls_stats`` at K = 21, 81, R = 300, A_NUM_CE_SAMPLE = 200: one thread per
               element / RoI at any K; recorded so the next reader knows whether they matter.

    python tools/uc_many_classes_bench.py [--out profiles/uc_many_classes.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.nets import uncertainty as U
    assert torch.cuda.is_available(), "uc_many_classes_bench needs the MI355X"
    dev = "cuda:0"
    C.reset_cfg()
    g = torch.Generator(device=dev).manual_seed(5)

    def event_time(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def alternate(fns, units):
        out = {k: [] for k in fns}
        for r in range(args.warmup + args.calls):
            for k, fn in fns.items():
                t = event_time(fn) / units
                if r >= args.warmup:
                    out[k].append(t)
        return {k: (float(np.median(v)), float(min(v))) for k, v in out.items()}

    def captured(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            keep = [fn() for _ in range(args.inner)]
        graph.keep = keep
        return graph

    def graph_us(fns):
        graphs = {n: captured(fn) for n, fn in fns.items()}
        t = alternate({n: gr.replay for n, gr in graphs.items()}, args.inner)
        return {n: "%.1f (%.1f)" % (v[0] * 1e6, v[1] * 1e6) for n, v in t.items()}, t

    lines = ["# The uncertainty heads at many classes (`tools/uc_many_classes_bench.py`)", "",
             "Command: `python tools/uc_many_classes_bench.py --out profiles/uc_many_classes.md`.  Every time is device time "
             "inside a captured hipGraph: %d calls per replay, median (minimum) of %d replays after %d warm-up replays, us per "
             "call unless stated." % (args.inner, args.calls, args.warmup)]

    # (a)
    n, s = 256, 200
    lines += ["", "## (a) Bayesian cross entropy, N = %d, S = %d, with gradients" % (n, s), "",
              "`narrow`: one thread per RoI (`frcnn_bayesian_cross_entropy`, K <= 16).  `wide`: one wave per RoI "
              "(`frcnn_bayesian_cross_entropy_wide`).  Both include the mean reduction (2 launches).", "",
              "| form | K | classes per lane | us per call |", "|---|---|---|---|"]
    for form, k in (("narrow", 2), ("narrow", 16), ("wide", 16), ("wide", 17), ("wide", 21), ("wide", 81)):
        score = torch.randn((n, k), device=dev, generator=g)
        logvar = torch.randn((n, k), device=dev, generator=g) * 0.7 - 0.5
        labels = torch.randint(0, k, (n,), device=dev, generator=g).float()
        fn = ops.bayesian_cross_entropy if form == "narrow" else ops.bayesian_cross_entropy_wide
        txt, _ = graph_us({"x": lambda: fn(score, logvar, labels, s, 11, 16, var_is_log=True)})
        cpl = "-" if form == "narrow" else str(next(c for c in (1, 2, 4, 8, 16) if c * 64 >= k))
        lines.append("| %s | %d | %s | %s |" % (form, k, cpl, txt["x"]))

    # (b)
    r, m, e = 300, 100, 4
    lines += ["", "## (b) Uncertainty columns, R = %d, %d rows per class, E = %d, eight sources" % (r, m, e), "",
              "`device`: `ops.uncertainty_columns` (1 launch).  `torch`: `stack_uncertainty_columns` + `torch.cat`, the "
              "statement it replaces.", "",
              "| K | output columns | device | torch | torch / device |", "|---|---|---|---|---|"]
    for k in (2, 4, 21, 81):
        rnd = lambda *sh: torch.randn(sh, device=dev, generator=g)
        unc = dict(a_entropy=rnd(r), a_mutual_info=rnd(r), a_cls_var=rnd(r, k), e_entropy=rnd(r), e_mutual_info=rnd(r),
                   e_cls_var=rnd(r, k), a_bbox_var=rnd(r, k * e), e_bbox_var=rnd(r, k * e))
        dets = rnd(k, m, e + 1)
        det_roi = torch.randint(0, r, (k, m), device=dev, generator=g).to(torch.int32)
        det_roi[:, m // 2:] = -1
        txt, t = graph_us({"device": lambda: U.append_uncertainty_columns(dets, unc, det_roi),
                           "torch": lambda: torch.cat((dets, U.stack_uncertainty_columns(unc, det_roi, k)), 2).contiguous()})
        lines.append("| %d | %d | %s | %s | %.1f |" % (k, e + 1 + 2 * (2 + k) + 2 * e, txt["device"], txt["torch"],
                                                       t["torch"][0] / t["device"][0]))

    # (d)
    lines += ["", "## (d) Untouched: `logit_distort` + `mc_cls_stats`, R = 300, A_NUM_CE_SAMPLE = 200", "",
              "| K | logit_distort + mc_cls_stats us |", "|---|---|"]
    for k in (21, 81):
        score = torch.randn((300, k), device=dev, generator=g)
        logvar = torch.randn((300, k), device=dev, generator=g) * 0.5

        def both():
            dist, var = ops.logit_distort(score, logvar, 200, 5, 15, var_is_log=True)
            return ops.mc_cls_stats(dist), var
        txt, _ = graph_us({"x": both})
        lines.append("| %d | %s |" % (k, txt["x"]))

    # (c)
    if not args.no_frame:
        from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
        from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
        from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
        h, w, k = 600, 1000, 21
        info = np.array([0, w, 0, h, 0, 0, 1.0], np.float32)
        blob = torch.from_numpy(bench.synthetic_frame(3)).to(dev)
        plans = os.path.join(ROOT, "profiles", bench.PLANS_FILE)
        if os.path.exists(plans):
            with open(plans) as f:
                ops.import_conv_plans(json.load(f))
        C.cfg.NET_TYPE = "image"
        for name in ("EN_BBOX_EPISTEMIC", "EN_CLS_EPISTEMIC", "EN_BBOX_ALEATORIC", "EN_CLS_ALEATORIC"):
            C.cfg.UC[name] = True
        net = imagenet(num_layers=101)
        net.create_architecture(k, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
        net.load_state_dict(seeded_state_dict(net, 7, bn_mode="tame"), strict=True)
        net.eval()
        net._device = dev
        net.to(dev)
        net.set_uc_seed(3)
        device_form = U.append_uncertainty_columns

        def torch_form(dets, uncertainties, det_roi):
            return torch.cat((dets, U.stack_uncertainty_columns(uncertainties, det_roi, k)), 2).contiguous()
        runners = {}
        for name, form in (("one launch", device_form), ("torch statement", torch_form)):
            U.append_uncertainty_columns = form
            try:
                runners[name] = FrameRunner(net, h, w, 3, info, thresh=1.0 / k, max_dets=bench.MAX_DETS, autotune=False)
                runners[name].run(blob)
                torch.cuda.synchronize()
            finally:
                U.append_uncertainty_columns = device_form
        res = {name: [] for name in runners}
        for rep in range(args.reps + 2):
            for name, rn in runners.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.frames):
                    rn.run(blob)
                torch.cuda.synchronize()
                if rep >= 2:
                    res[name].append((time.perf_counter() - t0) / args.frames)
        lines += ["", "## (c) The captured 1000 x 600 ResNet-101 TEST frame, 21 classes, all four `cfg.UC.EN_*` flags", "",
                  "One captured frame, filter included, E_NUM_SAMPLE = %d, A_NUM_CE_SAMPLE = %d, threshold 1 / K, max_dets %d; "
                  "host clock around %d replays ending in a device synchronise, per frame; median (minimum) of %d windows, "
                  "the two forms alternating.  `torch statement` is the frame with `stack_uncertainty_columns` + `torch.cat` "
                  "in place of the launch - the path before this change; nothing else differs." %
                  (int(C.cfg.UC.E_NUM_SAMPLE), int(C.cfg.UC.A_NUM_CE_SAMPLE), bench.MAX_DETS, args.frames, args.reps), "",
                  "| columns | ms per frame | frames/s |", "|---|---|---|"]
        for name, v in res.items():
            med = float(np.median(v))
            lines.append("| %s | %.3f (%.3f) | %.1f |" % (name, med * 1e3, min(v) * 1e3, 1 / med))
    C.reset_cfg()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
