#!/usr/bin/env python
"""A/B of the Winograd 3x3 convolution with and without the components that feed only dropped outputs
(frcnn_conv2d_set_algo 2 against 2 | 128), in ONE process, alternating the two forms.

    python tools/wino_trim_bench.py [--shape n,h,w,c,k]... [--tiles 6,12] [--streams 1,4] [--reps 40] [--rounds 9]

Per shape, GEMM tile (a plan tile index, forced through an imported Winograd plan row) and number of copies in flight, each
form is captured as one hipGraph of `reps` calls per stream (own activations and outputs per stream, the caller-supplied
filter transform as the detectors use it); the two sets of graphs are then replayed alternately `rounds` times, a host clock
around replays that end in a device synchronise.  Printed per form: fastest, median and slowest round in us per call, and
the rows the grouped GEMM executes (frcnn_conv2d_winograd_rows).
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from faster_rcnn_pytorch_multimodal_amd import _hip, ops                    # noqa: E402
from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import capture    # noqa: E402

FORMS = (("trimmed", 2), ("untrimmed", 2 | 128))


def build_graphs(mode, row, xs, ys, wt, u, sc, sh, reps):
    ops.set_conv_algo(mode)
    ops.import_conv_plans([row])
    run = lambda x, y: ops.conv2d_nhwc(x, wt, sc, sh, stride=1, pad=1, relu=True, out=y, w_winograd=u)
    for x, y in zip(xs, ys):
        run(x, y)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in xs]
    graphs = []
    for st, x, y in zip(streams, xs, ys):
        gr = torch.cuda.CUDAGraph()
        with capture(gr, stream=st):
            for _ in range(reps):
                run(x, y)
        graphs.append(gr)
    return streams, graphs


def replay(streams, graphs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for st, gr in zip(streams, graphs):
        with torch.cuda.stream(st):
            gr.replay()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], help="n,h,w,c,k (default: layer4's conv2 on 300 RoIs and 64x7x7 c256)")
    ap.add_argument("--tiles", default="6,12", help="plan tile indices of the grouped GEMM")
    ap.add_argument("--streams", default="1,4", help="copies in flight")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--untrimmed-first", action="store_true", help="capture and replay the untrimmed form first (order check)")
    args = ap.parse_args()
    forms = FORMS[::-1] if args.untrimmed_first else FORMS
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shape] or [(300, 7, 7, 512, 512), (64, 7, 7, 256, 256)]
    lib = _hip.load()
    g = torch.Generator().manual_seed(0)
    print("%-22s %4s %7s %-10s %8s %8s %8s %9s" % ("shape", "tile", "streams", "form", "min us", "med us", "max us", "GEMM rows"))
    for n, h, w, c, k in shapes:
        wt = (torch.randn(k, 3, 3, c, generator=g) / (3.0 * c ** 0.5)).cuda()
        sc, sh = (torch.rand(k, generator=g) + 0.5).cuda(), torch.randn(k, generator=g).cuda()
        u = ops.winograd_filter(wt)
        for tile in (int(t) for t in args.tiles.split(",")):
            row = [n, h, w, c, k, 3, 3, 1, 1, 1, tile + 16, 1, -(-c // 32)]
            for ns in (int(s) for s in args.streams.split(",")):
                xs = [torch.randn(n, h, w, c, generator=g).cuda() for _ in range(ns)]
                built, rows, outs = {}, {}, {}
                for name, mode in forms:
                    ys = [torch.empty(n, h, w, k, device="cuda") for _ in range(ns)]
                    built[name] = build_graphs(mode, row, xs, ys, wt, u, sc, sh, args.reps)
                    rows[name] = ops.winograd_rows(n, h, w)[1]
                    outs[name] = ys
                    replay(*built[name])                                        # warm replay
                times = {name: [] for name, _ in forms}
                for _ in range(args.rounds):
                    for name, _ in forms:
                        times[name].append(replay(*built[name]) / (args.reps * ns))
                same = all(torch.equal(a, b) for a, b in zip(outs["trimmed"], outs["untrimmed"]))
                for name, _ in forms:
                    t = sorted(times[name])
                    print("%-22s %4d %7d %-10s %8.1f %8.1f %8.1f %9d%s" % (
                        "%dx%dx%d c%d k%d" % (n, h, w, c, k), tile, ns, name, t[0], t[len(t) // 2], t[-1], rows[name],
                        "" if same else "  OUTPUTS DIFFER"), flush=True)
                del built
                _hip.check(lib.frcnn_conv2d_clear_plans(), "clear_plans")
    ops.set_conv_algo(0)


if __name__ == "__main__":
    main()
