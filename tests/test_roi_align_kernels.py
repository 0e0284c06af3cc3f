"""Every RoIAlign kernel form (csrc/roi_align.hip: generic, generic with XCD channel slices, planned with 8 / 4 loads in
flight, map-resident; backward through the plan and sample by sample, csrc/train_ops.hip) at its edges, each called through
ops.py and compared with a float64 reference that returns the linear operator of every RoI.

The reference (``roi_operator``) restates torchvision 0.4.0 roi_align (aligned=False): sample coordinates and every
comparison on them (< -1, > size, <= 0, >= size - 1, ceil, the int cast) follow the library's expression order in float32,
as O.roi_align does; interpolation weights from the float32 coordinate and all sums are float64.  Bilinear sampling
factorises per axis (a sample is dropped when EITHER coordinate is outside [-1, size]), so the operator of RoI r is
A_r = kron(Wy_r, Wx_r) / count_r, a dense (P*P, H*W) float64 matrix; forward = A @ F, backward = A^T @ dout.  The unmarked
tests check that reference against O.roi_align (another implementation, float32, not separable) and against float64
autograd through O.roi_align_torch, restate both kernel forms in float32 on the CPU (generic: O.roi_align; separable:
weights per axis, row sum, bin sum; backward: float32 accumulation in a few random orders) and require the bar with 4x
headroom, assert that every case reaches the regime it is named for, and apply to every boundary case the one-token
mutation of the restatement it exists to catch: the bar must then be exceeded.

Which case reaches which regime (case ids as pytest prints them):
  second trip of the plan's sample loop (grid > 64)      wide (grid_w 75, 64, 65), tall (grid_h 66), degenerate (65 x 58)
  second column chunk (bin wider than 64 columns)        wide (bins of 66 to 76 columns), forward and backward
  eight row chunks, first chunk the aligned one at 64    tall (rows 0..459; RoI 1 starts at row 70)
  variant 5 sample-by-sample path                        wide, degenerate (grid > 16), heavy_light (bins > 11 columns)
  prefix pass past 896 RoIs, second trip of t += stride  r1000 (975 items = 6825 wave-items > 5120 resident waves; an 8 x 8
                                                         map cannot hold a heavy RoI: rows_est * cols_est <= 64)
  channel tails, planned and generic                     c4 (one lane), c20 (no XCD split), c32 (one float4 per XCD slice),
                                                         c260 (second slice, one live lane), c320 (16 live), c512 (two full)
  channel slices of variant 5                            c16 c48 c128 c144 (1, 3, 8, 9 slices; nslices % 8 == 0 and != 0)
  split launch against the reference                     test_split_against_reference (split 256 of 260 and of 512)
  samples exactly at -1, 0, size-1, (size-1, size], size edges-s1, edges-s2 (and one ulp outside at -1 and size);
                                                         edges16-s1 / edges16-s2: corners x 16 at scale 1/16, bit-equal;
                                                         edges-s1-c16 / edges-s2-c16: the same boxes through variant 5
  whi == 0 weights: wc == 0 columns, !any rows           edges-s1 (integer samples, bin size 2: every other row / column)
  extent clamped to 1, zero-size box, box 50x the map    degenerate
  no valid sample on each of the four sides              degenerate (output exactly 0, no gradient)
  rows_est * cols_est exactly 64 / 65, pieces 1, 7, 0    heavy_light (with dead and other-level RoIs in one call)
  roi_count 0, R, R + 5; a level no RoI has              count0 countR countR5 nolevel
  other level's rows untouched                           every case with a level mask (heavy_light, r1000, nolevel) and
                                                         test_two_levels_write_one_output
  pooled 1, 2, 14                                        pooled1 pooled2 pooled14 (c = 8), pooled*-c6 (backward only)
  batch column                                           images2 (n = 2, maps differ, odd RoI count)
  per-image RoI blocks of variant 5                      blocks-3-0, blocks-0-2 (live counts per image, one of them 0)
  accumulation into a pre-filled dfeat                   test_backward_accumulates

Bars.  Index-like facts are exact: rows of RoIs on another level keep the sentinel bit for bit, dead RoIs and RoIs without
a valid sample are exactly zero, pixels no RoI touches keep exactly what they held, repeated forward calls are bit-equal.
Values: 2e-6 * max |reference| on both directions, the bars the suite already uses.  A bar the float32 restatement could
not meet with 4x headroom is listed in WIDENED with the measured error.

Refused by the map-resident kernel (an error, never wrong numbers): pooled != 7, c % 16 != 0, h > 64, a map slice that
does not fit the LDS, any epilogue.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import frcnn_oracle as O

DEV = "cuda:0"
F32 = np.float32
HEADROOM = 4.0
FRAC = 2e-6                          # of max |reference|: tests/test_gpu_parity.py, forward and planned-vs-per-sample backward
SENTINEL = -12345.6789               # what `out` holds before a forward call
HEAVY_LOADS = 64                     # g_roi_heavy_loads of csrc/roi_align.hip
PLAN_P = 7
ORDERS = 3                           # random summation orders of the float32 backward restatement
LIVE, DEAD, SKIP = 0, 1, 2
MUTATIONS = ("ge_size", "le_m1", "no_clamp", "drop_last", "floor_grid", "ignore_batch")

# (case, "fwd" | "bwd") -> (bar as a fraction of max |reference|, error of the float32 restatement that made FRAC too tight)
WIDENED = {
    ("r1000", "bwd"): (4.78e-06, 5.961e-05),        # 8 x 8 map, 926 live RoIs: ~3000 float32 atomics per pixel
    ("edges16-s2", "bwd"): (2.26e-06, 6.227e-06),   # one of the three orders; the other two stay below 2.9e-06        # 8 x 8 map, 926 live RoIs: ~3000 float32 atomics per pixel
}


def _ops():
    from faster_rcnn_pytorch_multimodal_amd import ops
    return ops


def _hip_mod():
    from faster_rcnn_pytorch_multimodal_amd import _hip
    return _hip


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ================================================================================================
# 1. the reference: the operator of every RoI
# ================================================================================================
def roi_geometry(rois, scale, sampling, pooled, mutation=None):
    """Float32 box arithmetic of the library kernel, for all RoIs at once."""
    r = np.asarray(rois, dtype=F32)
    sc, pf = F32(scale), F32(pooled)
    sw, sh, ew, eh = r[:, 1] * sc, r[:, 2] * sc, r[:, 3] * sc, r[:, 4] * sc
    rw, rh = np.maximum(ew - sw, F32(1.0)), np.maximum(eh - sh, F32(1.0))
    bw, bh = rw / pf, rh / pf
    rnd = np.floor if mutation == "floor_grid" else np.ceil
    if sampling > 0:
        gw = gh = np.full(r.shape[0], sampling, dtype=np.int64)
    else:
        gw, gh = np.maximum(rnd(rw / pf).astype(np.int64), 1), np.maximum(rnd(rh / pf).astype(np.int64), 1)
    assert all(a.dtype == F32 for a in (sw, sh, rw, rh, bw, bh))
    return dict(sw=sw, sh=sh, rw=rw, rh=rh, bw=bw, bh=bh, gw=gw, gh=gh)


def axis_samples(start, bin_size, grid, pooled, size, mutation=None):
    """Samples of one axis: v = start + p * bin + (i + .5) * bin / grid in float32 (R, P, I), which of them exist and are
    kept, their two pixels and the float32-coordinate the weights come from."""
    imax = int(grid.max())
    p = np.arange(pooled, dtype=F32)[None, :, None]
    i = np.arange(imax, dtype=F32)[None, None, :]
    s, b, g = start[:, None, None], bin_size[:, None, None], grid.astype(F32)[:, None, None]
    v = (s + p * b) + ((i + F32(0.5)) * b) / g
    assert v.dtype == F32
    idx = np.arange(imax)[None, None, :]
    exists = np.broadcast_to(idx < grid[:, None, None], v.shape).copy()
    if mutation == "drop_last":
        exists &= ~((idx % 64 == 63) | (idx == grid[:, None, None] - 1))
    below = v <= F32(-1.0) if mutation == "le_m1" else v < F32(-1.0)
    above = v >= F32(size) if mutation == "ge_size" else v > F32(size)
    keep = exists & ~below & ~above
    vc = np.where(keep, np.where(v <= 0, F32(0), v), F32(0)).astype(F32)
    lo = vc.astype(np.int64)                                   # the int cast truncates; vc >= 0
    top = lo >= size - 1
    if mutation == "no_clamp":                                 # pixels past the map read nothing
        hi = lo + 1
    else:
        lo = np.where(top, size - 1, lo)
        hi = np.where(top, size - 1, lo + 1)
        vc = np.where(top, lo.astype(F32), vc)
    return dict(v=v, exists=exists, keep=keep, lo=lo, hi=hi, vc=vc)


def axis_weights(smp, size, dtype):
    """W[r, p, pixel]: the weights of the kept samples summed per pixel in sample order (lo then hi), in ``dtype``."""
    lo, hi, vc, keep = smp["lo"], smp["hi"], smp["vc"], smp["keep"]
    if dtype == np.float64:
        whi = vc.astype(np.float64) - lo
        wlo = 1.0 - whi
    else:
        whi = vc - lo.astype(F32)
        wlo = F32(1.0) - whi
    r, p, n = lo.shape
    w = np.zeros((r, p, size + 2), dtype=dtype)
    ri, pi = np.meshgrid(np.arange(r), np.arange(p), indexing="ij")
    ri, pi = np.broadcast_to(ri[:, :, None, None], (r, p, n, 2)), np.broadcast_to(pi[:, :, None, None], (r, p, n, 2))
    px = np.stack((lo, hi), 3)
    wt = np.stack((wlo, whi), 3).astype(dtype)
    ok = np.broadcast_to(keep[..., None], px.shape) & (px < size)
    np.add.at(w, (ri[ok], pi[ok], px[ok]), wt[ok])
    return w[:, :, :size]


class Operator:
    """Wy (R, P, H), Wx (R, P, W), count (R,), img (R,), status (R,): A_r = kron(Wy_r, Wx_r) / count_r."""

    def __init__(self, spec, mutation=None, dtype=np.float64):
        rois = spec["rois"].numpy()
        geo = roi_geometry(rois, spec["scale"], spec["sampling"], spec["p"], mutation)
        self.geo = geo
        self.sx = axis_samples(geo["sw"], geo["bw"], geo["gw"], spec["p"], spec["w"], mutation)
        self.sy = axis_samples(geo["sh"], geo["bh"], geo["gh"], spec["p"], spec["h"], mutation)
        self.wx, self.wy = axis_weights(self.sx, spec["w"], dtype), axis_weights(self.sy, spec["h"], dtype)
        self.count = (geo["gw"] * geo["gh"]).astype(dtype)
        self.img, self.status = roi_images(spec, mutation), roi_status(spec)
        self.spec = spec

    def dense(self):
        r, p, h, w = len(self.count), self.spec["p"], self.spec["h"], self.spec["w"]
        a = np.einsum("rpy,rqx->rpqyx", self.wy, self.wx) / self.count[:, None, None, None, None]
        return a.reshape(r, p * p, h * w)

    def forward(self, feat):
        """feat (n, H, W, c) float64 -> (R, P, P, c); dead RoIs are zero, RoIs of another level nan (never written)."""
        p, c = self.spec["p"], feat.shape[3]
        fm = feat.reshape(feat.shape[0], -1, c)[self.img]
        out = np.einsum("rbk,rkc->rbc", self.dense(), fm).reshape(-1, p, p, c)
        out[self.status == DEAD] = 0.0
        out[self.status == SKIP] = np.nan
        return out

    def backward(self, dout, n):
        """dout (R, P, P, c) float64 -> dfeat (n, H, W, c): only live RoIs contribute."""
        p, c, h, w = self.spec["p"], dout.shape[3], self.spec["h"], self.spec["w"]
        a = self.dense() * (self.status == LIVE)[:, None, None]
        df = np.zeros((n, h * w, c))
        for b in range(n):
            sel = self.img == b
            df[b] = np.einsum("rbk,rbc->kc", a[sel], dout.reshape(-1, p * p, c)[sel])
        return df.reshape(n, h, w, c)

    def touched(self, n):
        """(n, H, W) bool: pixels some live RoI gives a non-zero weight."""
        a = (np.abs(self.dense()) * (self.status == LIVE)[:, None, None]).sum(1)
        t = np.zeros((n, self.spec["h"] * self.spec["w"]), dtype=bool)
        for b in range(n):
            t[b] = a[self.img == b].sum(0) > 0
        return t.reshape(n, self.spec["h"], self.spec["w"])


def roi_images(spec, mutation=None):
    r = spec["rois"].shape[0]
    if mutation == "ignore_batch":
        return np.zeros(r, dtype=np.int64)
    if spec["rpi"] > 0:
        return np.arange(r) // spec["rpi"]
    return spec["rois"][:, 0].numpy().astype(np.int64)


def roi_status(spec):
    r = spec["rois"].shape[0]
    st = np.full(r, LIVE)
    idx = np.arange(r)
    if spec["count"] is not None:
        if spec["rpi"] > 0:
            img = idx // spec["rpi"]
            st[(idx - img * spec["rpi"]) >= np.asarray(spec["count"])[img]] = DEAD
        else:
            st[idx >= min(int(spec["count"]), r)] = DEAD
    if spec["lvl"] is not None:
        st[np.asarray(spec["lvl"]) != spec["level"]] = SKIP                # the level is tested first
    return st


def roi_flag_products(spec):
    """rows_est * cols_est of roi_flag (csrc/roi_align.hip) in float32: above HEAVY_LOADS the RoI is split into row bins."""
    g = roi_geometry(spec["rois"].numpy(), spec["scale"], spec["sampling"], PLAN_P)
    rows = np.minimum(g["rh"].astype(np.int64) + 2, spec["h"])
    cols = np.minimum((g["rw"] / F32(PLAN_P)).astype(np.int64) + 2, spec["w"])
    return rows * cols


def plan_items(spec):
    """Pieces of the compact item list per RoI: 0 (other level), 1 (light or dead), 7 (heavy)."""
    st, heavy = roi_status(spec), roi_flag_products(spec) > HEAVY_LOADS
    return np.where(st == SKIP, 0, np.where((st == LIVE) & heavy, PLAN_P, 1))


def resident_ok(spec):
    lds = (spec["h"] * spec["w"] * 64 + 15) // 16 * 16 + 8 * 2 * 576 + 16
    return spec["p"] == PLAN_P and spec["c"] % 16 == 0 and spec["h"] <= 64 and spec["w"] <= 1024 and lds <= 160 * 1024


# ================================================================================================
# 2. the cases
# ================================================================================================
CASES = {}


def _add(name, h, w, c, rois, p=7, n=1, scale=1.0, sampling=0, count=None, lvl=None, level=-1, rpi=0, mutations=(),
         dirs="fb", regime=None):
    rois = torch.tensor(rois, dtype=torch.float64).float().contiguous()
    assert rois.ndim == 2 and rois.shape[1] == 5 and all(m in MUTATIONS for m in mutations)
    assert rpi > 0 or (0 <= int(rois[:, 0].min()) and int(rois[:, 0].max()) < n)        # the batch column indexes memory
    CASES[name] = dict(name=name, n=n, h=h, w=w, c=c, p=p, scale=scale, sampling=sampling, rois=rois, count=count,
                       lvl=lvl, level=level, rpi=rpi, mutations=tuple(mutations), dirs=dirs, regime=regime)


def _rand_rois(r, h, w, seed, n=1):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(r, 2, generator=g) * torch.tensor([w + 2.0, h + 2.0]) - 2.0
    wh = torch.rand(r, 2, generator=g) * torch.tensor([0.8 * w, 0.8 * h]) + 0.3
    b = torch.randint(0, n, (r, 1), generator=g).float()
    return torch.cat((b, xy, xy + wh), 1).tolist()


def _cols(smp):
    """Pixels a bin touches on one axis, (R, P): last pixel of the last kept sample - first pixel of the first + 1."""
    keep = smp["keep"]
    lo = np.where(keep, smp["lo"], 1 << 30).min(2)
    hi = np.where(keep, smp["hi"], -1).max(2)
    return np.where(keep.any(2), hi - lo + 1, 0), lo, hi


# ---- wide bins and large grids ------------------------------------------------------------------
def _regime_wide(d):
    op = d["op"]
    assert op.geo["gw"].tolist() == [75, 64, 65] and op.geo["gh"].tolist() == [1, 1, 1]
    cols, _, _ = _cols(op.sx)
    assert int(cols[0].max()) >= 75 and int(cols[1].min()) >= 65 and int(cols.min()) > 64       # a second column chunk
    assert bool((roi_flag_products(d["spec"]) > HEAVY_LOADS).all())
    assert resident_ok(d["spec"]) and int(op.geo["gw"].min()) > 16                             # variant 5: sample by sample


_add("wide", 4, 520, 16, [[0, 0, 0, 520, 4], [0, 10, 0, 458, 4], [0, 30.5, 0.5, 485.5, 3.5]],
     mutations=("drop_last",), regime=_regime_wide)


def _regime_tall(d):
    op = d["op"]
    assert op.geo["gh"].tolist() == [66, 56, 9] and op.geo["gw"].tolist() == [1, 1, 1]
    rows, lo, hi = _cols(op.sy)
    assert int(lo[0].min()) == 0 and int(hi[0].max()) == 459 and 459 // 64 == 7                 # row chunks 0..7
    assert int(lo[1].min()) == 70 and 70 & ~63 == 64                                            # first chunk is the one at 64
    assert int(rows[0].max()) > 64 and not resident_ok(d["spec"])


_add("tall", 460, 4, 8, [[0, 0, 0, 4, 460], [0, 0, 70, 4, 460], [0, 0.5, 100, 3.5, 163]],
     mutations=("drop_last",), regime=_regime_tall)


# ---- channel tails ------------------------------------------------------------------------------
CHANNELS = (4, 16, 20, 32, 48, 128, 144, 260, 320, 512)
_CH_ROIS = _rand_rois(10, 9, 11, 3) + [[0, -20, -2, 30, 12], [0, 0, 0, 11, 9]]


def _regime_channels(d):
    c = d["spec"]["c"]
    c4 = c // 4
    nslices = (c4 + 63) // 64
    live_last = c4 - 64 * (nslices - 1)
    want = {4: (1, 1), 20: (1, 5), 32: (1, 8), 260: (2, 1), 320: (2, 16), 512: (2, 64)}
    if c in want:
        assert (nslices, live_last) == want[c]
    assert (c % 32 == 0) == (c in (32, 128, 320, 512))                      # the XCD-split generic kernel
    assert resident_ok(d["spec"]) == (c % 16 == 0)
    if c in (16, 48, 128, 144):
        assert c // 16 == {16: 1, 48: 3, 128: 8, 144: 9}[c]
    flags = roi_flag_products(d["spec"]) > HEAVY_LOADS
    assert bool(flags.any()) and not bool(flags.all())


for _c in CHANNELS:
    _add("c%d" % _c, 9, 11, _c, _CH_ROIS, regime=_regime_channels)


# ---- exact boundaries ---------------------------------------------------------------------------
def _edge_ranges(size, s):
    d, last = 0.5 / s, 6 + (s - 0.5) / s             # bin size 1: first sample at start + d, last at start + last
    u1, u8 = 2.0 ** -23, 2.0 ** -20                  # spacing of float32 in [1, 2) and in [8, 16)
    return [(-1 - d, 6 - d),                         # 0: first sample exactly -1: kept, clamped to 0
            (-1 - d - u1, 6 - d),                    # 1: one ulp below -1: dropped (the width still rounds to 7)
            (size - last, size - last + 7),          # 2: last sample exactly at size: kept, clamped to size - 1
            (size - last + u8, size - last + 7 + u8),  # 3: one ulp above size: dropped
            (-d, 7 - d),                             # 4: first sample exactly 0
            (size - 1 - last, size - 1 - last + 7),  # 5: last sample exactly size - 1
            (size - 0.5 - last, size - 0.5 - last + 7),  # 6: last sample at size - .5, inside (size - 1, size]
            (-1.0, 13.0) if s == 1 else (-1.5, 12.5)]    # 7: bin size 2, integer samples (whi == 0)


def _edge_rois(s, mul=1.0):
    xs, ys = _edge_ranges(9, s), _edge_ranges(8, s)
    rois = [[0, a, 0.7, b, 6.3] for a, b in xs] + [[0, 1.2, a, 7.6, b] for a, b in ys]
    rois += [[0, xs[k][0], ys[k][0], xs[k][1], ys[k][1]] for k in (0, 2, 7)]
    return [[r[0]] + [v * mul for v in r[1:]] for r in rois]


def _regime_edges(d):
    op, s = d["op"], d["spec"]["sampling"]
    u1, u8 = F32(2.0 ** -23), F32(2.0 ** -20)
    for smp, size, base in ((op.sx, 9, 0), (op.sy, 8, 8)):
        v, keep = smp["v"], smp["keep"]
        first, last = (lambda k: (float(v[base + k, 0, 0]), bool(keep[base + k, 0, 0]))), \
                      (lambda k: (float(v[base + k, 6, s - 1]), bool(keep[base + k, 6, s - 1])))
        assert first(0) == (-1.0, True) and first(1) == (float(F32(-1) - u1), False)
        assert last(2) == (float(size), True) and last(3) == (float(F32(size) + u8), False)
        assert first(4) == (0.0, True) and last(5) == (size - 1.0, True) and last(6) == (size - 0.5, True)
        assert int(smp["lo"][base + 2, 6, s - 1]) == size - 1 and int(smp["lo"][base + 0, 0, 0]) == 0
        vi = v[base + 7][keep[base + 7]]
        assert bool((vi == np.round(vi)).all()) and vi.size > 4                       # integer samples: whi == 0
    if s == 1:                                         # zero-weight columns inside a bin's range, zero-weight rows
        wx, wy = op.wx[18], op.wy[18]
        assert bool((wx[:, 1::2] == 0).all()) and bool((wy[:, 1:6:2] == 0).all()) and float(wx[:, 0::2].sum()) > 0
    if d["spec"]["scale"] != 1.0:                      # corners x 16 at scale 1/16: the same float32 coordinates
        other = case_data(d["spec"]["name"].replace("edges16", "edges"))["op"]
        assert np.array_equal(op.sx["v"], other.sx["v"]) and np.array_equal(op.sy["v"], other.sy["v"])
        assert np.array_equal(op.dense(), other.dense())


for _s in (1, 2):
    _add("edges-s%d" % _s, 8, 9, 8, _edge_rois(_s), sampling=_s, mutations=("ge_size", "le_m1", "no_clamp"),
         regime=_regime_edges)
    _add("edges16-s%d" % _s, 8, 9, 8, _edge_rois(_s, 16.0), scale=1 / 16.0, sampling=_s,
         mutations=("ge_size", "le_m1", "no_clamp"), regime=_regime_edges)
    # the map-resident kernel has its own copy of the sample arithmetic and needs c % 16 == 0
    _add("edges-s%d-c16" % _s, 8, 9, 16, _edge_rois(_s), sampling=_s, mutations=("ge_size", "le_m1", "no_clamp"), dirs="f",
         regime=_regime_edges)


# ---- degenerate boxes ---------------------------------------------------------------------------
def _regime_degenerate(d):
    op = d["op"]
    g = op.geo
    assert float(g["rw"][0]) == 1.0 and float(g["rh"][0]) == 1.0 and float(g["rw"][1]) == 1.0 and float(g["rh"][1]) == 1.0
    assert int(op.sx["lo"][1][op.sx["keep"][1]].min()) == 8 and int(op.sy["lo"][1][op.sy["keep"][1]].min()) == 7
    assert int(g["gw"][2]) == 65 and int(g["gh"][2]) == 58 and roi_flag_products(d["spec"])[2] > HEAVY_LOADS
    assert (int(g["gw"][3]), int(g["gh"][3])) == (2, 2)                                # bin 1.5: floor would give 1
    dense = op.dense()
    for r in (4, 5, 6, 7):                             # outside on the left, right, top, bottom: every sample dropped
        assert not bool(dense[r].any())
    assert not bool(op.sx["keep"][4].any()) and not bool(op.sx["keep"][5].any())
    assert not bool(op.sy["keep"][6].any()) and not bool(op.sy["keep"][7].any())


_add("degenerate", 8, 9, 4, [[0, 6, 5, 2, 1], [0, 8, 7, 8, 7], [0, -200, -180, 250, 220], [0, -1, -1, 9.5, 9.5],
                             [0, -30, 1, -10, 5], [0, 20, 1, 30, 5], [0, 1, -30, 5, -10], [0, 1, 20, 5, 30]],
     mutations=("floor_grid",), regime=_regime_degenerate)


# ---- heavy / light at the default threshold -----------------------------------------------------
_HL_LVL = [0, 0, 1, 0, 0, 1, 0, 0]


def _regime_heavy_light(d):
    spec = d["spec"]
    assert roi_flag_products(spec).tolist() == [64, 64, 65, 65, 65, 64, 65, 64]
    assert roi_status(spec).tolist() == [LIVE, LIVE, SKIP, LIVE, LIVE, SKIP, DEAD, DEAD]
    assert plan_items(spec).tolist() == [1, 1, 0, 7, 7, 0, 1, 1]
    cols, _, _ = _cols(d["op"].sx)
    assert int(cols[4].max()) > 11                     # variant 5: a bin wider than its compact table


_add("heavy_light", 18, 30, 16,
     [[0, 2, 1, 18, 15.5], [0, 1, 3, 45, 9.5], [0, 3, 2, 26, 13.5], [0, 3, 2, 26, 13.5], [0, -30, 4, 50, 7.5],
      [0, 2, 1, 18, 15.5], [0, 3, 2, 26, 13.5], [0, 2, 1, 18, 15.5]],
     count=6, lvl=_HL_LVL, level=0, mutations=("floor_grid",), regime=_regime_heavy_light)


# ---- more than 896 RoIs -------------------------------------------------------------------------
_R1000_LVL = [2 if i % 40 == 7 else 1 for i in range(1000)]


def _regime_r1000(d):
    spec = d["spec"]
    items = plan_items(spec)
    assert len(items) == 1000 > 896 and int(roi_flag_products(spec).max()) <= HEAVY_LOADS
    assert sorted(set(items.tolist())) == [0, 1] and int(items.sum()) == 975
    st = roi_status(spec)
    assert int((st == DEAD).sum()) == 49 and int((st == SKIP).sum()) == 25 and int((st[897:] == LIVE).sum()) > 40
    # the persistent grids hold min(256 * 5, ceil(49 R / 4)) workgroups of 4 waves
    waves = 4 * min(256 * 5, (1000 * 49 + 3) // 4)
    assert waves == 5120 < int(items.sum()) * PLAN_P < 2 * waves       # second trip, and the prefetch runs past the end


_add("r1000", 8, 8, 4, _rand_rois(1000, 8, 8, 11), count=950, lvl=_R1000_LVL, level=1, regime=_regime_r1000)


# ---- counts and masks ---------------------------------------------------------------------------
_CM_ROIS = _rand_rois(6, 9, 11, 5)


def _regime_counts(d):
    spec, st = d["spec"], roi_status(d["spec"]).tolist()
    want = {"count0": [DEAD] * 6, "countR": [LIVE] * 6, "countR5": [LIVE] * 6, "nolevel": [SKIP] * 6}[spec["name"]]
    assert st == want
    if spec["name"] == "nolevel":
        assert int(plan_items(spec).sum()) == 0                       # total_items == 0


_add("count0", 9, 11, 16, _CM_ROIS, sampling=2, count=0, regime=_regime_counts)
_add("countR", 9, 11, 16, _CM_ROIS, sampling=2, count=6, regime=_regime_counts)
_add("countR5", 9, 11, 16, _CM_ROIS, sampling=2, count=11, regime=_regime_counts)
_add("nolevel", 9, 11, 16, _CM_ROIS, sampling=2, lvl=[0, 1, 2, 0, 1, 2], level=7, regime=_regime_counts)


# ---- pooled 1, 2, 14 ----------------------------------------------------------------------------
def _regime_pooled(d):
    spec = d["spec"]
    assert spec["p"] != PLAN_P and not resident_ok(spec) and d["op"].dense().shape[1] == spec["p"] ** 2
    assert spec["c"] % 4 == 0 or spec["dirs"] == "b"


for _p in (1, 2, 14):
    _add("pooled%d" % _p, 9, 11, 8, _CH_ROIS, p=_p, regime=_regime_pooled)
    _add("pooled%d-c6" % _p, 9, 11, 6, _CH_ROIS, p=_p, dirs="b", regime=_regime_pooled)


# ---- several images -----------------------------------------------------------------------------
_IMG_ROIS = [[b] + r[1:] for b, r in zip([0, 1, 1, 0, 1, 0, 1], _rand_rois(7, 9, 11, 8))]


def _regime_images(d):
    spec, op = d["spec"], d["op"]
    assert spec["n"] == 2 and len(op.img) % 2 == 1                    # odd: one half wave of variant 5 has no partner
    if spec["rpi"] == 0:
        assert op.img.tolist() == [0, 1, 1, 0, 1, 0, 1]
    else:
        assert op.img.tolist() == [0, 0, 0, 0, 1, 1, 1] and bool((spec["rois"][:, 0] == 0).all())
        live = [int(((op.status == LIVE) & (op.img == b)).sum()) for b in (0, 1)]
        assert live == list(spec["count"]) and 0 in live
    assert float((d["feat"][0] - d["feat"][1]).abs().min()) > 0                        # the two maps differ everywhere


_add("images2", 9, 11, 16, _IMG_ROIS, n=2, mutations=("ignore_batch",), regime=_regime_images)
_BLK_ROIS = [[0] + r[1:] for r in _IMG_ROIS]                          # the batch column says 0: the position decides
_add("blocks-3-0", 9, 11, 16, _BLK_ROIS, n=2, rpi=4, count=(3, 0), dirs="f", regime=_regime_images)
_add("blocks-0-2", 9, 11, 16, _BLK_ROIS, n=2, rpi=4, count=(0, 2), dirs="f", mutations=("ignore_batch",),
     regime=_regime_images)

CASE_IDS = list(CASES)
FWD_CASES = [k for k in CASE_IDS if "f" in CASES[k]["dirs"]]
BWD_CASES = [k for k in CASE_IDS if "b" in CASES[k]["dirs"]]
MUTATION_CASES = [(k, m) for k in CASE_IDS for m in CASES[k]["mutations"]]


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs and float64 references of a case, computed once and shared (read only)."""
    spec = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))        # stable when cases are added
    r, p, c = spec["rois"].shape[0], spec["p"], spec["c"]
    feat = torch.randn(spec["n"], spec["h"], spec["w"], c, generator=g)
    dout = torch.randn(r, p, p, c, generator=g)
    op = Operator(spec)
    fwd = op.forward(feat.double().numpy())
    bwd = op.backward(dout.double().numpy(), spec["n"])
    return dict(spec=spec, feat=feat, dout=dout, op=op, fwd=fwd, bwd=bwd)


def _bar(name, direction, ref):
    frac = WIDENED.get((name, direction), (FRAC,))[0]
    live = ref[np.isfinite(ref)]
    return frac * (float(np.abs(live).max()) if live.size else 0.0)


def _check(name, direction, side, got, ref, headroom=1.0):
    """max |got - ref| over the entries the reference defines, against the bar; prints the figure first."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref)
    assert got.shape == ref.shape, (name, direction, side, got.shape, ref.shape)
    mask = np.isfinite(ref)
    assert bool(np.isfinite(got[mask]).all()), (name, direction, side, "result not finite")
    err = float(np.abs(got[mask] - ref[mask]).max()) if mask.any() else 0.0
    bar = _bar(name, direction, ref)
    print("RAK|%s|%s|%s|err=%.3e|bar=%.3e|ratio=%.4f" % (name, direction, side, err, bar, err / bar if bar else 0.0))
    assert err * headroom <= bar, "%s %s (%s): max err %.3e, bar %.3e / %g" % (name, direction, side, err, bar, headroom)
    return err


def _effective_rois(spec, op):
    rois = spec["rois"].clone()
    rois[:, 0] = torch.from_numpy(op.img).float()
    return rois


def _mask_status(out, status):
    out = np.array(out, dtype=np.float64)
    out[status == DEAD] = 0.0
    out[status == SKIP] = np.nan
    return out


# ================================================================================================
# 3. CPU: the reference, the bars, the regimes, the mutations
# ================================================================================================
@pytest.mark.parametrize("name", CASE_IDS)
def test_reference_forward_matches_oracle(name):
    """O.roi_align (float32, sample by sample: the generic kernels' restatement) meets the forward bar with 4x headroom."""
    d = case_data(name)
    spec, op = d["spec"], d["op"]
    got = O.roi_align(d["feat"].permute(0, 3, 1, 2).contiguous(), _effective_rois(spec, op), spec["p"], spec["scale"],
                      spec["sampling"]).permute(0, 2, 3, 1).numpy()
    _check(name, "fwd", "oracle32", _mask_status(got, op.status), d["fwd"], HEADROOM)


@pytest.mark.parametrize("name", CASE_IDS)
def test_cpu_restatement_separable_forward(name):
    """The planned and map-resident kernels' arithmetic in float32: weights per axis, row sum, bin sum, 1 / count."""
    d = case_data(name)
    spec = d["spec"]
    op32 = Operator(spec, dtype=F32)
    fm = d["feat"][torch.from_numpy(op32.img)]                                          # (R, H, W, c)
    rows = torch.einsum("rqx,ryxc->rqyc", torch.from_numpy(op32.wx), fm)
    out = torch.einsum("rpy,rqyc->rpqc", torch.from_numpy(op32.wy), rows)
    out = out * torch.from_numpy(F32(1.0) / op32.count)[:, None, None, None]
    assert out.dtype == torch.float32
    _check(name, "fwd", "separable32", _mask_status(out.numpy(), op32.status), d["fwd"], HEADROOM)


@pytest.mark.parametrize("name", CASE_IDS)
def test_reference_backward_matches_autograd(name):
    d = case_data(name)
    spec, op = d["spec"], d["op"]
    rois = _effective_rois(spec, op)
    dout = d["dout"].double() * torch.from_numpy(op.status == LIVE)[:, None, None, None]
    got = np.zeros_like(d["bwd"])
    for b in range(spec["n"]):
        sel = torch.from_numpy(op.img == b)
        if not bool(sel.any()):
            continue
        f = d["feat"][b:b + 1].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        out = O.roi_align_torch(f, rois[sel], spec["p"], spec["scale"], spec["sampling"])         # (R, C, P, P)
        out.backward(dout[sel].permute(0, 3, 1, 2))
        got[b] = f.grad[0].permute(1, 2, 0).numpy()
    _check(name, "bwd", "autograd64", got, d["bwd"])


def _per_sample_contributions(spec, op32, dout):
    """(pixel index, value) of every atomic of the sample-by-sample backward, float32: g * (wy * wx), g = dout / count."""
    h, w, c, p = spec["h"], spec["w"], spec["c"], spec["p"]
    idx, val = [], []
    for r in np.nonzero(op32.status == LIVE)[0]:
        gh, gw = int(op32.geo["gh"][r]), int(op32.geo["gw"][r])
        g = dout[r].numpy() / F32(gh * gw)                                              # (P, P, c)
        ax = []
        for smp, n in ((op32.sy, gh), (op32.sx, gw)):
            lo, hi, vc, keep = (smp[k][r, :, :n] for k in ("lo", "hi", "vc", "keep"))
            whi = vc - lo.astype(F32)
            ax.append((np.stack((lo, hi), 2), np.stack((F32(1.0) - whi, whi), 2), keep))
        (py, wy, ky), (px, wx, kx) = ax                                                  # (P, n, 2)
        pix = (py[:, :, :, None, None, None] * w + px[None, None, None]) + int(op32.img[r]) * h * w   # (P,gh,2,P,gw,2)
        wgt = wy[:, :, :, None, None, None] * wx[None, None, None]
        ok = np.broadcast_to(ky[:, :, None, None, None, None] & kx[None, None, None, :, :, None], pix.shape)
        gg = np.broadcast_to(g[:, None, None, :, None, None, :], pix.shape + (c,))
        idx.append(pix[ok])
        val.append(gg[ok] * wgt[ok][:, None])
    if not idx:
        return np.zeros(0, dtype=np.int64), np.zeros((0, c), dtype=F32)
    return np.concatenate(idx), np.concatenate(val).astype(F32)


def _planned_contributions(spec, op32, dout):
    """One (image, T (H, c), wx (W,)) per wave-item of the planned backward: T = sum_ph wy[ph] * g[ph][pw] in float32 (all
    row bins of a light RoI, one of a heavy RoI); the item adds wx[x] * T[y] to pixel (y, x)."""
    heavy = roi_flag_products(spec) > HEAVY_LOADS if spec["p"] == PLAN_P else np.zeros(len(op32.count), dtype=bool)
    items = []
    for r in np.nonzero(op32.status == LIVE)[0]:
        g = dout[r].numpy() * (F32(1.0) / op32.count[r])                                 # (P, P, c)
        for pw in range(spec["p"]):
            if heavy[r]:
                for ph in range(spec["p"]):
                    items.append((int(op32.img[r]), op32.wy[r, ph][:, None] * g[ph, pw][None, :], op32.wx[r, pw]))
            else:
                t = np.zeros((spec["h"], spec["c"]), dtype=F32)
                for ph in range(spec["p"]):
                    t = t + op32.wy[r, ph][:, None] * g[ph, pw][None, :]
                items.append((int(op32.img[r]), t, op32.wx[r, pw]))
    return items


@pytest.mark.parametrize("name", BWD_CASES)
def test_cpu_restatement_backward(name):
    """Both backward forms in float32 on the CPU, the atomics in ORDERS random orders: the largest error keeps 4x headroom."""
    d = case_data(name)
    spec = d["spec"]
    n, h, w, c = spec["n"], spec["h"], spec["w"], spec["c"]
    op32 = Operator(spec, dtype=F32)
    idx, val = _per_sample_contributions(spec, op32, d["dout"])
    items = _planned_contributions(spec, op32, d["dout"])
    worst = 0.0
    for seed in range(ORDERS):
        rng = np.random.default_rng(seed)
        acc = np.zeros((n * h * w, c), dtype=F32)
        order = rng.permutation(len(idx))
        np.add.at(acc, idx[order], val[order])
        worst = max(worst, _check(name, "bwd", "per-sample32 order %d" % seed, acc.reshape(n, h, w, c), d["bwd"], HEADROOM))
        acc = np.zeros((n, h, w, c), dtype=F32)
        for k in rng.permutation(len(items)):
            b, t, wx = items[k]
            nz = np.nonzero(wx)[0]
            acc[b][:, nz] += wx[None, nz, None] * t[:, None, :]
        worst = max(worst, _check(name, "bwd", "planned32 order %d" % seed, acc, d["bwd"], HEADROOM))
    assert acc.dtype == F32


@pytest.mark.parametrize("name", CASE_IDS)
def test_case_reaches_its_regime(name):
    d = case_data(name)
    assert d["spec"]["regime"] is not None
    d["spec"]["regime"](d)
    assert bool(np.isfinite(d["bwd"]).all())


@pytest.mark.parametrize("name,mutation", MUTATION_CASES, ids=["%s-%s" % km for km in MUTATION_CASES])
def test_mutation_exceeds_bar(name, mutation):
    """The one-token mutation the case exists to catch moves the forward result past the case's bar."""
    d = case_data(name)
    got = Operator(d["spec"], mutation=mutation).forward(d["feat"].double().numpy())
    mask = np.isfinite(d["fwd"])
    err = float(np.abs(got[mask] - d["fwd"][mask]).max())
    bar = _bar(name, "fwd", d["fwd"])
    print("RAK|%s|mutation %s|err=%.3e|bar=%.3e" % (name, mutation, err, bar))
    assert err > bar, (name, mutation, err, bar)
    dgot = Operator(d["spec"], mutation=mutation).backward(d["dout"].double().numpy(), d["spec"]["n"])
    assert float(np.abs(dgot - d["bwd"]).max()) > _bar(name, "bwd", d["bwd"]) or "b" not in d["spec"]["dirs"]


def test_every_mutation_has_a_case():
    assert {m for _, m in MUTATION_CASES} == set(MUTATIONS)


def test_widened_bars_keep_their_headroom():
    for (name, direction), (frac, err) in WIDENED.items():
        assert name in CASES and direction in ("fwd", "bwd") and frac > FRAC
        ref = case_data(name)[direction]
        assert HEADROOM * err <= frac * float(np.abs(ref[np.isfinite(ref)]).max()) * 1.001, (name, direction)


# ================================================================================================
# 4. GPU
# ================================================================================================
def _variants(spec):
    if spec["rpi"] > 0:
        return [5]                                     # per-image RoI blocks exist in the map-resident kernel only
    return [1, 2, 3, 4, 0] + ([5] if resident_ok(spec) else [])


FWD_RUNS = [(k, v) for k in FWD_CASES for v in _variants(CASES[k])]


def _dev_args(spec):
    cnt = None if spec["count"] is None else torch.tensor(np.atleast_1d(spec["count"]), dtype=torch.int32, device=DEV)
    lvl = None if spec["lvl"] is None else torch.tensor(spec["lvl"], dtype=torch.int32, device=DEV)
    return dict(roi_count=cnt, level_of_roi=lvl, level=spec["level"])


def _forward(hip, spec, feat, rois, variant, out=None, **kw):
    ops = _ops()
    r, p, c = rois.shape[0], spec["p"], feat.shape[3]
    if out is None:
        out = torch.full((r, p, p, c), SENTINEL, dtype=torch.float32, device=DEV)
    hip.frcnn_roi_align_set_variant(variant)
    try:
        ops.roi_align_nhwc(feat, rois, p, spec["scale"], spec["sampling"], out=out, rois_per_image=spec["rpi"],
                           **dict(_dev_args(spec), **kw))
        torch.cuda.synchronize()
    finally:
        hip.frcnn_roi_align_set_variant(0)
    return out


def _check_forward(name, side, out, d):
    op, ref = d["op"], d["fwd"]
    out = out.cpu()
    sent = torch.full_like(out[0], SENTINEL)
    for r in np.nonzero(op.status == SKIP)[0]:
        assert _bits_equal(out[r], sent), (name, side, "RoI %d of another level was written" % r)
    dead = torch.from_numpy(op.status == DEAD)
    assert bool((out[dead] == 0).all()), (name, side, "dead RoIs are not zero")
    empty = torch.from_numpy((op.status == LIVE) & ~op.dense().any(axis=(1, 2)))
    assert bool((out[empty] == 0).all()), (name, side, "a RoI without a valid sample is not zero")
    _check(name, "fwd", side, out.numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", FWD_RUNS, ids=["%s-v%d" % kv for kv in FWD_RUNS])
def test_forward(hip, name, variant):
    d = case_data(name)
    spec = d["spec"]
    feat, rois = d["feat"].to(DEV), spec["rois"].to(DEV)
    out = _forward(hip, spec, feat, rois, variant)
    _check_forward(name, "variant %d" % variant, out, d)
    assert _bits_equal(out, _forward(hip, spec, feat, rois, variant))                   # deterministic
    if name.startswith("edges16"):                    # the same float32 coordinates as at scale 1: the same bits
        other = case_data(name.replace("edges16", "edges"))
        assert _bits_equal(out, _forward(hip, other["spec"], feat, other["spec"]["rois"].to(DEV), variant))


BWD_RUNS = [(k, f) for k in BWD_CASES for f in (True, False)]


def _backward(spec, dout, rois, planned, dfeat=None):
    ops = _ops()
    old = ops.ROI_ALIGN_BWD_PLANNED
    ops.ROI_ALIGN_BWD_PLANNED = planned
    try:
        got = ops.roi_align_bwd(dout, (spec["n"], spec["h"], spec["w"], spec["c"]), rois, spec["scale"], spec["sampling"],
                                dfeat=dfeat, **_dev_args(spec))
        torch.cuda.synchronize()
    finally:
        ops.ROI_ALIGN_BWD_PLANNED = old
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name,planned", BWD_RUNS, ids=["%s-%s" % (k, "planned" if f else "per-sample") for k, f in BWD_RUNS])
def test_backward(hip, name, planned):
    """Both settings of ROI_ALIGN_BWD_PLANNED; pooled != 7, c % 4 != 0 and n > 1 fall back to the sample-by-sample kernel
    as ops.roi_align_bwd documents."""
    d = case_data(name)
    spec = d["spec"]
    got = _backward(spec, d["dout"].to(DEV), spec["rois"].to(DEV), planned).cpu()
    untouched = torch.from_numpy(~d["op"].touched(spec["n"]))
    assert bool((got[untouched] == 0).all()), (name, "a pixel no RoI touches received a gradient")
    _check(name, "bwd", "planned" if planned else "per-sample", got.numpy(), d["bwd"])


@pytest.mark.gpu
@pytest.mark.parametrize("planned", [True, False], ids=["planned", "per-sample"])
@pytest.mark.parametrize("name", ["c20", "c260", "heavy_light"])
def test_backward_accumulates(hip, name, planned):
    """dfeat that already holds values: the result is prefill + reference (the prefill is dyadic, so the first addition to
    a pixel is exact up to the rounding of the sum, which the bar on max |prefill + reference| covers)."""
    d = case_data(name)
    spec = d["spec"]
    g = torch.Generator().manual_seed(4)
    prefill = torch.randint(-8, 9, (spec["n"], spec["h"], spec["w"], spec["c"]), generator=g).float() / 4
    got = _backward(spec, d["dout"].to(DEV), spec["rois"].to(DEV), planned, dfeat=prefill.clone().to(DEV)).cpu()
    untouched = torch.from_numpy(~d["op"].touched(spec["n"]))
    assert _bits_equal(got[untouched], prefill[untouched])
    ref = prefill.double().numpy() + d["bwd"]
    err = float(np.abs(got.double().numpy() - ref).max())
    bar = FRAC * float(np.abs(ref).max())
    print("RAK|%s|bwd accumulate|%s|err=%.3e|bar=%.3e" % (name, "planned" if planned else "per-sample", err, bar))
    assert err <= bar


def test_cpu_restatement_backward_accumulates():
    """The same accumulation in float32 on the CPU keeps 4x headroom under the bar of test_backward_accumulates."""
    for name in ("c20", "c260", "heavy_light"):
        d = case_data(name)
        spec = d["spec"]
        g = torch.Generator().manual_seed(4)
        shape = (spec["n"], spec["h"], spec["w"], spec["c"])
        prefill = torch.randint(-8, 9, shape, generator=g).float() / 4
        ref = prefill.double().numpy() + d["bwd"]
        idx, val = _per_sample_contributions(spec, Operator(spec, dtype=F32), d["dout"])
        for seed in range(ORDERS):
            acc = prefill.numpy().reshape(-1, spec["c"]).copy()
            order = np.random.default_rng(seed).permutation(len(idx))
            np.add.at(acc, idx[order], val[order])
            assert HEADROOM * float(np.abs(acc.reshape(shape) - ref).max()) <= FRAC * float(np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("c", [260, 512])
def test_split_against_reference(hip, c):
    """roi_align_split (one plan, two launches over channel ranges) against the reference, not against another launch;
    with an epilogue, RoIs beyond the count hold exactly act(shift)."""
    ops = _ops()
    d = case_data("c%d" % c)
    spec = d["spec"]
    feat, rois = d["feat"].to(DEV), spec["rois"].to(DEV)
    out1, out2 = ops.roi_align_split(feat, rois, 7, spec["scale"], 256, spec["sampling"])
    got = torch.cat((out1, out2), 3).cpu()
    assert out1.shape[3] == 256 and out2.shape[3] == c - 256
    _check("c%d" % c, "fwd", "split 256", got.numpy(), d["fwd"])
    g = torch.Generator().manual_seed(c)
    scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    cnt = torch.tensor([9], dtype=torch.int32, device=DEV)
    e1, e2 = ops.roi_align_split(feat, rois, 7, spec["scale"], 256, spec["sampling"], roi_count=cnt, scale=scale.to(DEV),
                                 shift=shift.to(DEV), relu1=True)
    want = torch.cat((torch.clamp_min(out1.cpu() * scale[:256] + shift[:256], 0.0), out2.cpu() * scale[256:] + shift[256:]), 3)
    act_shift = torch.cat((torch.clamp_min(shift[:256], 0.0), shift[256:]))
    got_e = torch.cat((e1, e2), 3).cpu()
    assert torch.equal(got_e[:9], want[:9])                                            # the same pooled values, bit for bit
    assert torch.equal(got_e[9:], act_shift.expand(got_e.shape[0] - 9, 7, 7, c))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 0, 5])
def test_two_levels_write_one_output(hip, variant):
    """Two pyramid levels (maps of different size and scale) pooled into one output, as the FPN path does: every row equals
    the reference of its own level."""
    rois = _rand_rois(9, 18, 22, 12)
    lvl = [0, 1, 1, 0, 1, 0, 0, 1, 1]
    levels = ((9, 11, 0.5, 0), (18, 22, 1.0, 1))
    out = torch.full((9, 7, 7, 16), SENTINEL, dtype=torch.float32, device=DEV)
    ref = np.full((9, 7, 7, 16), np.nan)
    for h, w, scale, level in levels:
        spec = dict(name="levels", n=1, h=h, w=w, c=16, p=7, scale=scale, sampling=2, count=None, lvl=lvl, level=level,
                    rpi=0, rois=torch.tensor(rois, dtype=torch.float32))
        feat = torch.randn(1, h, w, 16, generator=torch.Generator().manual_seed(level))
        mine = Operator(spec).forward(feat.double().numpy())
        ref[np.asarray(lvl) == level] = mine[np.asarray(lvl) == level]
        _forward(hip, spec, feat.to(DEV), spec["rois"].to(DEV), variant, out=out)
    assert bool(np.isfinite(ref).all())
    _check("levels", "fwd", "variant %d" % variant, out.cpu().numpy(), ref)


@pytest.mark.gpu
def test_refusals(hip):
    """What has no map-resident or planned form is an error or the documented fall-back, never another kernel's numbers
    under the wrong name."""
    ops, err = _ops(), _hip_mod().HipError
    for name in ("pooled2", "c20", "tall"):                                            # pooled != 7, c % 16 != 0, h > 64
        d = case_data(name)
        assert not resident_ok(d["spec"])
        with pytest.raises(err):
            _forward(hip, d["spec"], d["feat"].to(DEV), d["spec"]["rois"].to(DEV), 5)
    d = case_data("blocks-3-0")                                                        # per-image blocks: variant 5 only
    for variant in (0, 1, 3):
        with pytest.raises(err):
            _forward(hip, d["spec"], d["feat"].to(DEV), d["spec"]["rois"].to(DEV), variant)
    d = case_data("pooled2")                                                           # the planned backward refuses ...
    spec = d["spec"]
    dout, rois = d["dout"].to(DEV), spec["rois"].to(DEV)
    dfeat = torch.zeros(1, spec["h"], spec["w"], spec["c"], device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    rc = hip.frcnn_roi_align_bwd_planned(ops._ptr(dout), spec["h"], spec["w"], spec["c"], ops._ptr(rois), None, rois.shape[0],
                                         2, 1.0, 0, None, -1, ops._ptr(dfeat), ops._ptr(ws), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    assert rc != 0 and not bool(dfeat.any())
    assert hip.frcnn_roi_align_fwd_ws_bytes(spec["h"], spec["w"], spec["c"], rois.shape[0], 2) == 0     # ... ops falls back
