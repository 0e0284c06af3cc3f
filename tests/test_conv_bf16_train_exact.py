"""The two bf16 training convolutions of cfg.TRAIN.CONV_BF16 through ``ops``, bit for bit against float64 on the host, with
every operand, the output and the workspace between guard bands:

  * the filter gradient - conv_wgrad_bf16 in conv_wgrad.hip, entered through frcnn_conv2d_bwd_weight_bf16 / _acc_bf16 in
    conv_wgrad_plan.hip, finished by wgrad_reduce_kernel / wgrad_accumulate_kernel and the fp32 bias gradient;
  * the data gradient - frcnn_conv2d_bwd_data_bf16 in conv_dgrad.hip: dilate_kernel, ONE frcnn_conv2d_fwd_bf16 launch of dy
    with the bf16 pack of the flipped, transposed filter (pad_t = r - 1 - pad), frcnn_act_bwd in place on dx.

Method (that of test_conv_f32_exact.py and test_conv_bf16_exact.py).  Operands are integers held in fp32:

    regime  first operand                  second operand                 what it pins
    T1      ints in [-3, 3]                ints in [-3, 3]                the sum itself: every term present, once, at the right index
    T2      odd, 256 <= |v| < 1024         ints in [-2, 2]                the first operand is rounded to bf16, nearest even
    T3      ints in [-2, 2]                odd, 256 <= |v| < 1024         the same for the second operand

(first, second) = (x, dy) for the filter gradient and (dy, w) for the data gradient.  Every odd integer in [256, 512) is a tie
between two bf16 neighbours (257 -> 256, 259 -> 260); in [512, 1024) 4q + 1 rounds down and 4q + 3 up.  The reference is the
float64 definition (E.dw_float64 / E.dx_float64) on rbf16(operand), the host's float32 -> bfloat16 -> float64 cast.  Rounded
magnitudes are at most 1024 and the reductions at most 4608 terms, so every partial sum in any order - and "before + 2 dw" of
the accumulating form - stays below 2^24: the comparison is equality.  ``test_regime_precondition_holds`` asserts that per case.
The bias gradient is the fp32 sum of the UNROUNDED dy.

Buffers.  Outputs and workspaces are views between NaN bands of E.BAND floats, NaN-filled before the call, the workspace of
exactly the bytes the ``*_ws_bytes`` query answers for that call; x, dy, add, act_y, act_scale, the gradient accumulated into
and grad_b lie between NaN bands, the packed filter between bands of the bf16 NaN word.  After the call: bands intact, no NaN
in the result (an element never written, or a consumed read outside an operand), result == float64.

``emulate_wgrad`` / ``emulate_dgrad`` are host emulations of the two operations with the split, tap, carry, layout, dilation
and epilogue steps explicit; they equal the float64 definition on every small case, and each one-line change of MUTATIONS
changes the result of the case listed beside it (no GPU needed).

A NEW FORM OF EITHER KERNEL - A TILE, A SPLIT RULE, A FUSED EPILOGUE ON THE DATA GRADIENT, ANOTHER STORE PATH - MUST BE ADDED
TO THE LISTS BELOW (REQUESTS, TILES, STORE_PATHS, EPILOGUES, W_NEW / D_NEW).  profiles/conv_bf16_train_exact_tests.md has the
case tables, the grid caps, the mutation list and the measured time.
"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

import test_conv_f32_exact as E
from guarded_buffers import DEV, guarded, guards_flag
from test_conv_bf16_exact import _ints, _odd, guarded_copy, guarded_words, hooks, plane_bits, word_bands_flag
from test_conv_wgrad_bf16 import rbf16

BAND = E.BAND
TWO24 = 1 << 24
NAN = float("nan")
REGIMES = ("T1", "T2", "T3")
ODD10 = _odd(256, 1024)
GENERATORS = {"T1": (_ints(3), _ints(3)), "T2": (ODD10, _ints(2)), "T3": (_ints(2), ODD10)}       # (first, second) operand
TILES = (1, 2)                   # set_conv_bf16_tile on the data gradient's forward launch: 64x64, 128x128
STORE_PATHS = (0, 64)            # set_conv_algo: LDS transpose; stores straight from the MFMA layout
EPILOGUES = ("none", "add", "add_y", "add_y_scale")

BR = 32                          # conv_wgrad.h: pixels per reduction step
BIAS_GROUPS = 64                 # conv_wgrad.h: rows of the bias gradient's partial sums
THREADS = 256                    # every kernel below runs 256 threads per workgroup
REDUCE_CAP = 4096                # launch_reduce, conv_wgrad.hip: min((n4 + 255) / 256, 4096) workgroups, 16 bytes per thread
ACCUMULATE_CAP = 8192            # run_wgrad, conv_wgrad_plan.hip: launch_accumulate(..., 8192, stream), one gradient element per thread
DILATE_CAP = 8192                # frcnn_conv2d_bwd_data_bf16, conv_dgrad.hip: min((total + 255) / 256, 8192), 16 bytes per thread
TRANSPOSE_CAP = 4096             # frcnn_conv2d_transpose_filter, conv_dgrad.hip: min((total + 255) / 256, 4096), one element per thread
# (frcnn_conv2d_pack_bf16, conv_bf16.hip, has no cap and no loop: (count + 255) / 256 workgroups, one element per thread)

# ---- case tables: name -> (n, h, w, c, k, r, stride, pad) -------------------------------------------------------------------------
W_NEW = {
    "c36_k68_3x3": (1, 5, 7, 36, 68, 3, 1, 1),         # Q = 324 over three Q tiles, taps change inside a tile, both edges ragged, no multiples of 32
    "c8_k4_3x3": (1, 4, 5, 8, 4, 3, 1, 1),             # 16 taps' worth of chunks in one Q tile; K = 4: one chunk of dy
    "stem_creal3": E.SHAPES["stem"],                   # the accumulating form into (64, 3, 7, 7) from a C = 4 operand
    "tiny_maps": (9, 1, 5, 32, 32, 1, 1, 0),           # 5-pixel maps: d_img = 6, d_rem = 2
    "column": (3, 11, 1, 32, 32, 3, 1, 1),             # Wo == 1
    "row_wide": (1, 2, 40, 32, 32, 3, 1, 1),           # Wo > 32: d_ho == 0
    "m64_exact": (1, 8, 8, 32, 32, 1, 1, 0),           # M an exact multiple of 32
    "m33": (1, 3, 11, 32, 32, 1, 1, 0),                # a last step of one pixel
    "five_steps": (1, 10, 16, 32, 32, 1, 1, 0),        # 160 pixels: a request for 4 splits runs 3
    # K Q = 4.2 M floats, 33 pixels: with two splits wgrad_reduce_kernel gets 4105 > REDUCE_CAP workgroups' worth of 16-byte
    # elements, wgrad_accumulate_kernel 16416 > ACCUMULATE_CAP workgroups' worth of gradient elements - both loop
    "reduce_stride": (1, 3, 11, 2048, 2052, 1, 1, 0),
}
W_SHAPES = {**E.SHAPES, **W_NEW}
C_REAL = {"stem_creal3": 3}
W_ONCE = ("layer3", "persistent")                      # T1, the library's own split count, both forms
REQUESTS = lambda steps: (1, 2, 3, 5, steps, steps + 1)

D_NEW = {
    "c36_out": (1, 5, 7, 36, 64, 3, 1, 1),             # the forward launch's K = 36: ragged on both tiles
    "c4_out_5x5": (1, 9, 6, 4, 32, 5, 1, 2),           # K = 4, 25 taps
    # E's 3x3s2_even has k = 48, which this entry point refuses (k % 32, asserted below): the same map at k = 64, the one
    # shape here whose zero-inserted map has a remainder row and column
    "3x3s2_even_k64": (2, 8, 10, 32, 64, 3, 2, 1),
    # n hd wd k / 4 = 181 181 72 = 2 358 792 > DILATE_CAP x 256 = 2 097 152 (k = 256: 2 096 704, just short): dilate_kernel loops
    "dilate_stride": (1, 181, 181, 32, 288, 3, 2, 1),
    # 512 x 3 x 3 x 256 = 1 179 648 filter elements > TRANSPOSE_CAP x 256 = 1 048 576: transpose_filter_kernel loops; 4608 workgroups of the packer
    "filter_stride": (1, 3, 3, 256, 512, 3, 1, 1),
}
D_FROM_F32 = {name: sh for name, sh in E.SHAPES.items() if sh[4] % 32 == 0 and not (sh[5] == 1 and sh[6] > 1)}
D_SHAPES = {**D_FROM_F32, **D_NEW}
D_BIG = ("layer3", "dilate_stride", "filter_stride")   # the library's tile and the default store path only
REFUSED = "3x3s2_even"                                 # k = 48

W_CASES = [("wgrad", name, regime) for name in W_SHAPES for regime in (("T1",) if name in W_ONCE else REGIMES)]
D_CASES = [("dgrad", name, regime) for name in D_SHAPES for regime in REGIMES]
CASES = W_CASES + D_CASES
W_SMALL = [name for name in W_SHAPES if name not in W_ONCE and name != "reduce_stride"]
D_SMALL = [name for name in D_SHAPES if name not in D_BIG]


def case_id(c):
    return "%s-%s-%s" % c


# ---- the float64 definitions: E's, lent a shape this file adds -------------------------------------------------------------------
_LENT = "(a shape of test_conv_bf16_train_exact.py)"


def _lend(fn, shape, *args):
    """E.dw_float64 / E.dx_float64 look their geometry up by name: E.SHAPES holds ``shape`` under a private name for the call."""
    E.SHAPES[_LENT] = shape
    try:
        return fn(_LENT, *args)
    finally:
        del E.SHAPES[_LENT]


def dw64(shape, x, dy):
    return _lend(E.dw_float64, shape, x, dy)


def dx64(shape, dy, wt):
    return _lend(E.dx_float64, shape, dy, wt)


def trunc_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (toward zero), as float64: the conversion a kernel must NOT apply."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def geometry(shape):
    n, h, w, c, k, r, stride, pad = shape
    ho, wo = E.out_hw(h, w, r, stride, pad)
    return ho, wo, n * ho * wo


def steps_of(shape):
    return (geometry(shape)[2] + BR - 1) // BR


def effective_splits(steps, requested):
    """bf16_plan in conv_wgrad_plan.hip for a caller's count > 0: clamped to the steps, then to the count that leaves no empty range."""
    sp = max(1, min(requested, steps))
    per = (steps + sp - 1) // sp
    return (steps + per - 1) // per


def split_requests(shape):
    """One request per effective split count, the smallest that gives it."""
    seen, out = set(), []
    for req in REQUESTS(steps_of(shape)):
        eff = effective_splits(steps_of(shape), req)
        if eff not in seen:
            seen.add(eff)
            out.append(req)
    return out


def wgrad_ws_bytes_host(shape, splits):
    """frcnn_conv2d_bwd_weight_bf16_ws_bytes for ``splits`` effective splits: the slabs (one at least: the accumulating form
    reduces from the workspace), 256-aligned, then the bias partials."""
    n, h, w, c, k, r, stride, pad = shape
    slab = k * r * r * c * 4
    return (max(splits if splits > 1 else 0, 1) * slab + 255) // 256 * 256 + BIAS_GROUPS * k * 4


def _generator(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(key).encode()))


@functools.lru_cache(maxsize=None)
def wgrad_case(name, regime):
    """Operands (fp32) and float64 results of one filter-gradient case, computed once and left unchanged.  T1 on a shape of
    test_conv_f32_exact.py is that file's reference: same x and dy, one float64 filter gradient for both files."""
    shape = W_SHAPES[name]
    n, h, w, c, k, r, stride, pad = shape
    ho, wo, m = geometry(shape)
    c_real = C_REAL.get(name, c)
    g = _generator("wgrad", name, regime)
    if regime == "T1" and name in E.SHAPES:
        ref = E.reference(name)
        x, dy, dw = ref["x"].float(), ref["dy"].float(), ref["dw"]
    else:
        make_x, make_dy = GENERATORS[regime]
        x, dy = make_x((n, h, w, c), g), make_dy((n, ho, wo, k), g)
        dw = dw64(shape, rbf16(x), rbf16(dy))
    db = dy.double().reshape(-1, k).sum(0)
    before, before_b = _ints(5)((k, c_real, r, r), g).double(), _ints(5)((k,), g).double()
    return {"x": x, "dy": dy, "dw": dw, "db": db, "before": before, "before_b": before_b, "c_real": c_real,
            "acc": (before + 2.0 * dw.permute(0, 3, 1, 2)[:, :c_real]).contiguous(), "acc_b": before_b + 2.0 * db}


def dx_wanted(dx, add, act_y, act_scale, epilogue):
    if epilogue == "none":
        return dx
    v = dx + add
    if epilogue == "add":
        return v
    if epilogue == "add_y_scale":
        v = v * act_scale
    return torch.where(act_y > 0, v, torch.zeros_like(v))


@functools.lru_cache(maxsize=None)
def dgrad_case(name, regime):
    """Operands (fp32) and float64 results of one data-gradient case.  act_y holds 0.0, -0.0, positive and negative values in
    equal parts, act_scale powers of two in [1/4, 4]."""
    shape = D_SHAPES[name]
    n, h, w, c, k, r, stride, pad = shape
    ho, wo, m = geometry(shape)
    g = _generator("dgrad", name, regime)
    if regime == "T1" and name in E.SHAPES:
        ref = E.reference(name)
        dy, wt, dx = ref["dy"].float(), ref["w"].float(), ref["dx"]
    else:
        make_dy, make_w = GENERATORS[regime]
        dy, wt = make_dy((n, ho, wo, k), g), make_w((k, r, r, c), g)
        dx = dx64(shape, rbf16(dy), rbf16(wt))
    add = _ints(3)((n, h, w, c), g)
    mag = torch.randn((n, h, w, c), generator=g).abs() + 0.5
    kind = torch.randint(0, 4, (n, h, w, c), generator=g)
    act_y = torch.where(kind == 0, mag, torch.where(kind == 1, -mag, torch.where(kind == 2, torch.zeros(()), -torch.zeros(()))))
    act_scale = (2.0 ** torch.randint(-2, 3, (c,), generator=g).double()).float()
    out = {"dy": dy, "w": wt, "add": add, "act_y": act_y, "act_scale": act_scale, "dx": dx}
    out["want"] = {e: dx_wanted(dx, add.double(), act_y.double(), act_scale.double(), e) for e in EPILOGUES}
    return out


# ---- host emulations, the kernels' steps explicit -----------------------------------------------------------------------------------
def pixel_walk(shape, step_begin, step_end, mutation=None):
    """The pixels (m, img, ho, wo) conv_wgrad_bf16's threads stage for steps [step_begin, step_end): per pixel group pg the
    state starts from a division, walks four pixels by ++ carries, and advances one step by (d_img, d_ho, d_wo) and one carry each."""
    n, h, w, c, k, r, stride, pad = shape
    Ho, Wo, M = geometry(shape)
    d_img = BR // (Ho * Wo)
    d_rem = BR - d_img * Ho * Wo
    d_ho = d_rem // Wo
    d_wo = d_rem - d_ho * Wo
    limit = (M // BR) * BR if mutation == "tail_pixels_dropped" else M
    out = []
    for pg in range(8):
        m = step_begin * BR + pg * 4
        img = m // (Ho * Wo)
        rem = m - img * Ho * Wo
        ho = rem // Wo
        wo = rem - ho * Wo
        for _ in range(step_begin, step_end):
            mi, ii, hh, ww = m, img, ho, wo
            for _i in range(4):
                if mi < limit:
                    out.append((mi, ii, hh, ww))
                mi += 1
                ww += 1
                if ww == Wo:
                    ww = 0
                    hh += 1
                    if hh == Ho:
                        hh = 0
                        ii += 1
            m += BR
            wo += d_wo
            ho += d_ho
            img += d_img
            if wo >= Wo:
                wo -= Wo
                ho += 1
            if ho >= Ho:
                ho -= Ho
                if mutation != "image_carry_dropped":
                    img += 1
    return out


def emulate_wgrad(shape, ops_, splits, mutation=None):
    """{"dw" (k,r,s,c), "acc" (k,c_real,r,s) after two accumulating calls, "db", "acc_b"} in float64 with ``splits`` effective
    splits: rounding, the per-slab pixel walk, tap = q / C, the padding test, the gather from x's flat memory (a row past the
    last image is a NaN band), the slab sum in z order, krsc_index and the accumulation."""
    n, h, w, c, k, r, stride, pad = shape
    Ho, Wo, M = geometry(shape)
    x, dy, c_real = ops_["x"], ops_["dy"], ops_["c_real"]
    xr = {"x_truncated": trunc_bf16(x), "x_unrounded": x.double()}.get(mutation, rbf16(x))
    dyr = {"dy_truncated": trunc_bf16(dy), "dy_unrounded": dy.double()}.get(mutation, rbf16(dy))
    xflat = torch.cat([xr.reshape(-1, c), torch.full((w, c), NAN, dtype=torch.float64)])
    Q = r * r * c
    q = torch.arange(Q)
    tap = q // c
    cb = q - tap * c
    tr = tap // r
    ts = tap - tr * r
    if mutation == "r_s_exchanged":
        tr, ts = ts, tr
    steps = steps_of(shape)
    per = (steps + splits - 1) // splits
    slabs = []
    for z in range(splits):
        walk = pixel_walk(shape, z * per, min((z + 1) * per, steps), mutation)
        slab = torch.zeros((k, Q), dtype=torch.float64)
        if walk:
            mi, ii, hh, ww = (torch.tensor(col) for col in zip(*walk))
            hi = hh[:, None] * stride - pad + tr[None, :]
            wi = ww[:, None] * stride - pad + ts[None, :]
            h_ok = (hi >= 0) & ((hi <= h) if mutation == "padding_bound_hi_le_H" else (hi < h))
            ok = h_ok & (wi >= 0) & (wi < w)
            row = ((ii[:, None] * h + hi) * w + wi).clamp(0, xflat.shape[0] - 1)
            patch = torch.where(ok, xflat[row, cb[None, :].expand_as(row)], torch.zeros((), dtype=torch.float64))
            slab = dyr.reshape(-1, k)[mi].t() @ patch
        slabs.append(slab)
    if mutation == "last_slab_left_out" and splits > 1:
        slabs = slabs[:-1]
    total = slabs[0].clone()
    for slab in slabs[1:]:
        total = total + slab
    # the accumulating form: element i of (k, c_real, r, s) reads krsc_index(i) of the (k, r, s, c) result
    i = torch.arange(k * c_real * r * r)
    s_ = i % r
    t = i // r
    r_ = t % r
    t = t // r
    lay = c if mutation == "C_for_c_real" else c_real
    src = (((t // lay) * r + r_) * r + s_) * c + t % lay
    v = total.reshape(-1)[src]
    grad = ops_["before"].reshape(-1).clone()
    for _ in range(2):
        grad = v.clone() if mutation == "accumulate_overwrites" else grad + v
    db = (rbf16(dy) if mutation == "bias_from_rounded_dy" else dy.double()).reshape(-1, k).sum(0)
    return {"dw": total.view(k, r, r, c), "acc": grad.view(k, c_real, r, r), "db": db, "acc_b": ops_["before_b"] + 2.0 * db}


def emulate_dgrad(shape, ops_, epilogue, mutation=None):
    """dx (n,h,w,c) in float64: rounding, the flipped and transposed filter, zero insertion with the remainder rows and columns,
    a stride-1 convolution padded by pad_t written row-major into dx's memory (NaN where nothing is written), add, mask, scale."""
    n, h, w, c, k, r, stride, pad = shape
    ho, wo, m = geometry(shape)
    dyr = trunc_bf16(ops_["dy"]) if mutation == "dy_truncated" else rbf16(ops_["dy"])
    wt = rbf16(ops_["w"])
    flipped = wt if mutation == "filter_not_flipped" else wt.flip(1, 2)
    w_t = flipped.contiguous().reshape(c, r, r, k) if mutation == "filter_not_transposed" else flipped.permute(3, 1, 2, 0)
    pad_t = pad if mutation == "pad_t_is_pad" else r - 1 - pad
    src = dyr
    if stride > 1 and r > 1:
        rem_h, rem_w = (0, 0) if mutation == "remainder_dropped" else ((h + 2 * pad - r) % stride, (w + 2 * pad - r) % stride)
        src = torch.zeros((n, (ho - 1) * stride + 1 + rem_h, (wo - 1) * stride + 1 + rem_w, k), dtype=torch.float64)
        src[:, 0:(ho - 1) * stride + 1:stride, 0:(wo - 1) * stride + 1:stride] = dyr
    y = F.conv2d(src.permute(0, 3, 1, 2), w_t.permute(0, 3, 1, 2), padding=pad_t).permute(0, 2, 3, 1).reshape(-1)
    flat = torch.full((n * h * w * c,), NAN, dtype=torch.float64)
    count = min(flat.numel(), y.numel())
    flat[:count] = y[:count]
    v = flat.view(n, h, w, c)
    add, act_y, scale = ops_["add"].double(), ops_["act_y"].double(), ops_["act_scale"].double()
    if epilogue == "none":
        return v
    if epilogue == "add":
        return v + add
    is_open = act_y >= 0 if mutation == "mask_is_ge_0" else act_y > 0
    zero = torch.zeros_like(v)
    if mutation == "mask_before_add":
        v = torch.where(is_open, v, zero) + add
        return v * scale if epilogue == "add_y_scale" else v
    v = v + add
    if epilogue == "add_y_scale":
        v = v * scale
    return torch.where(is_open, v, zero)


# ---- CPU: the inputs are valid, independently of the kernels ---------------------------------------------------------------------
def test_host_rounding_is_nearest_even_and_truncation_is_not():
    v = torch.tensor([257.0, 259.0, 261.0, 263.0, 513.0, 515.0, 1021.0, 1023.0, -257.0, -259.0])
    assert rbf16(v).tolist() == [256.0, 260.0, 260.0, 264.0, 512.0, 516.0, 1020.0, 1024.0, -256.0, -260.0]
    odd = torch.arange(257, 1024, 2).float()
    assert bool((rbf16(odd) != odd.double()).all()) and float(rbf16(odd).max()) == 1024.0
    differ = float((trunc_bf16(odd) != rbf16(odd)).double().mean())
    assert 0.45 < differ < 0.55, differ
    assert bool((trunc_bf16(-odd) == -trunc_bf16(odd)).all())


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_regime_precondition_holds(c):
    """sum |rbf16(a)| |rbf16(b)| (+ |add|) < 2^24, also for the twice-accumulated gradient; the large operand of T2 / T3 really
    is rounded (every element of it), the small operands are not; the float64 results are fp32 numbers."""
    grad, name, regime = c
    if grad == "wgrad":
        shape, ops_ = W_SHAPES[name], wgrad_case(name, regime)
        a, b = ops_["x"], ops_["dy"]
        assert shape[3] % 4 == 0 and shape[4] % 4 == 0
        mag = dw64(shape, rbf16(a).abs(), rbf16(b).abs())
        assert float(mag.max()) < TWO24
        assert float((2.0 * mag.permute(0, 3, 1, 2)[:, :ops_["c_real"]] + ops_["before"].abs()).max()) < TWO24
        assert float((2.0 * b.double().abs().reshape(-1, shape[4]).sum(0) + ops_["before_b"].abs()).max()) < TWO24
        results = [ops_["dw"], ops_["acc"], ops_["db"], ops_["acc_b"]]
    else:
        shape, ops_ = D_SHAPES[name], dgrad_case(name, regime)
        a, b = ops_["dy"], ops_["w"]
        assert shape[3] % 4 == 0 and shape[4] % 32 == 0
        assert float((dx64(shape, rbf16(a).abs(), rbf16(b).abs()) + ops_["add"].double().abs()).max()) < TWO24
        y = ops_["act_y"]
        zeros = y == 0
        assert bool((zeros & torch.signbit(y)).any()) and bool((zeros & ~torch.signbit(y)).any()) and bool((y > 0).any()) and bool((y < 0).any())
        assert bool(((ops_["act_scale"] >= 0.25) & (ops_["act_scale"] <= 4.0)).all())
        results = list(ops_["want"].values())
    for t in results:
        assert torch.equal(t.float().double(), t)
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    for operand, large in ((a, regime == "T2"), (b, regime == "T3")):
        if large:
            assert bool((rbf16(operand) != operand.double()).all()) and float(rbf16(operand).abs().max()) <= 1024.0
        else:
            assert torch.equal(rbf16(operand), operand.double())


def test_split_requests_are_reclamped_as_bf16_plan_does():
    """five_steps: a request for 4 runs 3 (2 steps per slab); steps + 1 runs steps; every shape's list of requests gives
    distinct effective counts, 1 among them, and the workspace query answers for the CLAMPED count."""
    lib = E.lib()
    five = W_SHAPES["five_steps"]
    assert steps_of(five) == 5 and effective_splits(5, 4) == 3 and effective_splits(5, 6) == 5
    assert [effective_splits(5, req) for req in split_requests(five)] == [1, 2, 3, 5]
    n, h, w, c, k, r, stride, pad = five
    query = lambda sh, req: int(lib.frcnn_conv2d_bwd_weight_bf16_ws_bytes(sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], sh[5], sh[6], sh[7], req))
    assert query(five, 4) == query(five, 3) == wgrad_ws_bytes_host(five, 3) != wgrad_ws_bytes_host(five, 4)
    for name, shape in W_SHAPES.items():
        steps = steps_of(shape)
        effs = [effective_splits(steps, req) for req in split_requests(shape)]
        assert effs[0] == 1 and len(set(effs)) == len(effs) and max(effs) == steps
        for req in REQUESTS(steps):
            assert query(shape, req) == wgrad_ws_bytes_host(shape, effective_splits(steps, req)), (name, req)


def test_the_grid_caps_are_exceeded():
    """reduce_stride, dilate_stride and filter_stride give each capped launch more than its cap's worth of work."""
    n, h, w, c, k, r, stride, pad = W_SHAPES["reduce_stride"]
    assert steps_of(W_SHAPES["reduce_stride"]) == 2 and 2 in [effective_splits(2, q) for q in split_requests(W_SHAPES["reduce_stride"])]
    assert (k * r * r * c // 4 + THREADS - 1) // THREADS > REDUCE_CAP                    # launch_reduce's n4 = K Q / 4
    assert (k * c * r * r + THREADS - 1) // THREADS > ACCUMULATE_CAP                     # launch_accumulate's total = K c_real R S
    n, h, w, c, k, r, stride, pad = D_SHAPES["dilate_stride"]
    ho, wo, m = geometry(D_SHAPES["dilate_stride"])
    hd, wd = (ho - 1) * stride + 1 + (h + 2 * pad - r) % stride, (wo - 1) * stride + 1 + (w + 2 * pad - r) % stride
    assert (hd, wd) == (181, 181)
    assert (n * hd * wd * (k // 4) + THREADS - 1) // THREADS > DILATE_CAP >= (n * hd * wd * (256 // 4) + THREADS - 1) // THREADS
    n, h, w, c, k, r, stride, pad = D_SHAPES["filter_stride"]
    assert (k * r * r * c + THREADS - 1) // THREADS == 4608 > TRANSPOSE_CAP


def test_the_case_tables_reach_what_they_claim():
    assert sorted(D_FROM_F32) == sorted(["3x3_pad0", "3x3s2_pad0", "3x3s2_odd", "stem", "3x3_map1", "3x3_odd_batch", "linear", "layer3"])
    assert E.SHAPES[REFUSED][4] == 48
    rem = lambda sh: ((sh[1] + 2 * sh[7] - sh[5]) % sh[6], (sh[2] + 2 * sh[7] - sh[5]) % sh[6])
    assert rem(D_SHAPES["3x3s2_even_k64"]) == (1, 1) and D_SHAPES["3x3s2_even_k64"][:4] == E.SHAPES[REFUSED][:4]
    assert [name for name, sh in D_SHAPES.items() if sh[5] - 1 - sh[7] != sh[7]] == ["3x3_pad0", "3x3s2_pad0"]      # pad_t != pad
    assert {D_SHAPES[name][3] % 32 for name in ("c36_out", "c4_out_5x5", "stem")} == {4}
    geo = {name: geometry(sh) for name, sh in W_SHAPES.items()}
    assert geo["linear"][:2] == (1, 1) and geo["column"][1] == 1 and geo["3x3_map1"][2] == 1 and geo["one_pixel"][2] == 1
    assert geo["row_wide"][1] > BR and geo["m64_exact"][2] == 64 and geo["m33"][2] == 33 and geo["five_steps"][2] == 160
    ho, wo, m = geo["tiny_maps"]
    assert (BR // (ho * wo), BR % (ho * wo)) == (6, 2)
    n, h, w, c, k, r, stride, pad = W_SHAPES["c36_k68_3x3"]
    assert r * r * c == 324 and (r * r * c) % 32 and k % 32 and 128 // c >= 3                    # a 128-wide Q tile holds more than three taps
    assert max(sh[5] for sh in W_SHAPES.values()) == 7 and "5x5" in W_SHAPES and "3x3_pad0" in W_SHAPES and "3x3s2_pad0" in W_SHAPES
    assert max(geometry(sh)[2] for sh in W_SHAPES.values()) == 2394                              # the bound of the docstring
    assert max(sh[4] * sh[5] * sh[5] for sh in D_SHAPES.values()) == 4608


@pytest.mark.parametrize("name", W_SMALL)
def test_filter_gradient_emulation_equals_float64(name):
    """The emulation with its explicit walk, taps, slabs and layout IS the definition, in every regime and at every split count."""
    shape = W_SHAPES[name]
    for regime in REGIMES:
        ops_ = wgrad_case(name, regime)
        for req in split_requests(shape):
            got = emulate_wgrad(shape, ops_, effective_splits(steps_of(shape), req))
            for key in ("dw", "acc", "db", "acc_b"):
                assert torch.equal(got[key], ops_[key]), (name, regime, req, key)


@pytest.mark.parametrize("name", D_SMALL)
def test_data_gradient_emulation_equals_float64(name):
    shape = D_SHAPES[name]
    for regime in REGIMES:
        ops_ = dgrad_case(name, regime)
        for epilogue in EPILOGUES:
            assert torch.equal(emulate_dgrad(shape, ops_, epilogue), ops_["want"][epilogue]), (name, regime, epilogue)


# mutation -> (gradient, case of the tables that stops equalling float64, regime, what is compared)
MUTATIONS = {
    "x_truncated": ("wgrad", "c36_k68_3x3", "T2", "dw"),
    "dy_truncated": ("wgrad", "c36_k68_3x3", "T3", "dw"),
    "x_unrounded": ("wgrad", "c36_k68_3x3", "T2", "dw"),
    "dy_unrounded": ("wgrad", "c36_k68_3x3", "T3", "dw"),
    "tail_pixels_dropped": ("wgrad", "c36_k68_3x3", "T1", "dw"),
    "r_s_exchanged": ("wgrad", "c36_k68_3x3", "T1", "dw"),
    "padding_bound_hi_le_H": ("wgrad", "3x3_odd_batch", "T1", "dw"),
    "image_carry_dropped": ("wgrad", "3x3_odd_batch", "T1", "dw"),
    "last_slab_left_out": ("wgrad", "five_steps", "T1", "dw"),
    "accumulate_overwrites": ("wgrad", "c8_k4_3x3", "T1", "acc"),
    "C_for_c_real": ("wgrad", "stem_creal3", "T1", "acc"),
    "bias_from_rounded_dy": ("wgrad", "c36_k68_3x3", "T3", "db"),
    "filter_not_flipped": ("dgrad", "3x3_odd_batch", "T1", "none"),
    "filter_not_transposed": ("dgrad", "3x3_odd_batch", "T1", "none"),
    "pad_t_is_pad": ("dgrad", "3x3_pad0", "T1", "none"),
    "remainder_dropped": ("dgrad", "3x3s2_even_k64", "T1", "none"),
    "mask_before_add": ("dgrad", "3x3_odd_batch", "T1", "add_y"),
    "mask_is_ge_0": ("dgrad", "3x3_odd_batch", "T1", "add_y"),
    "dy_truncated_dgrad": ("dgrad", "c36_out", "T2", "none"),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_one_line_arithmetic_changes_are_caught(mutation):
    """Each change, emulated on the host, changes the float64 result of a case the device tests run (at every split count of
    that case for the filter gradient; "last slab left out" at every count above 1)."""
    grad, name, regime, key = MUTATIONS[mutation]
    if grad == "wgrad":
        shape, ops_ = W_SHAPES[name], wgrad_case(name, regime)
        for req in split_requests(shape):
            eff = effective_splits(steps_of(shape), req)
            assert torch.equal(emulate_wgrad(shape, ops_, eff)[key], ops_[key])
            wrong = emulate_wgrad(shape, ops_, eff, mutation)[key]
            differ = int((wrong != ops_[key]).sum())
            print("%s: %s %s, %d splits: %d of %d elements of %s differ from float64" % (mutation, name, regime, eff, differ, wrong.numel(), key))
            # (a slab of one step starts from a division and never carries; one slab has no last slab to leave out)
            seen = {"last_slab_left_out": eff > 1, "image_carry_dropped": eff < steps_of(shape)}.get(mutation, True)
            assert (differ > 0) == seen
    else:
        shape, ops_ = D_SHAPES[name], dgrad_case(name, regime)
        assert torch.equal(emulate_dgrad(shape, ops_, key), ops_["want"][key])
        wrong = emulate_dgrad(shape, ops_, key, mutation.replace("_dgrad", ""))
        differ = int((wrong != ops_["want"][key]).sum())
        print("%s: %s %s, epilogue %s: %d of %d elements differ from float64" % (mutation, name, regime, key, differ, wrong.numel()))
        assert differ > 0


# ---- guarded device runs ---------------------------------------------------------------------------------------------------------
def operands_flag(dev):
    return torch.stack([guards_flag(buf, numel, BAND) for buf, numel in dev["bufs"]]
                       + [word_bands_flag(buf, numel) for buf, numel in dev.get("wbufs", [])]).all()


@functools.lru_cache(maxsize=None)
def wgrad_on_device(name, regime):
    ops_ = wgrad_case(name, regime)
    dev = {"bufs": []}
    for key in ("x", "dy"):
        buf, dev[key] = guarded_copy(ops_[key])
        dev["bufs"].append((buf, ops_[key].numel()))
    for key in ("dw", "db", "acc", "acc_b"):
        dev[key] = ops_[key].to(DEV)
    for key in ("before", "before_b"):
        dev[key] = ops_[key].float().to(DEV)
    return dev


def run_wgrad(name, regime, requested):
    """One split request: the plain form into a NaN-filled (k,r,s,c) view with the bias gradient, then the accumulating form
    twice into a (k,c_real,r,s) view and a grad_b view that hold values.  Returns the number of library calls."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    shape = W_SHAPES[name]
    n, h, w, c, k, r, stride, pad = shape
    dev = wgrad_on_device(name, regime)
    c_real = C_REAL.get(name, c)
    ws_bytes = ops.conv2d_bwd_weight_bf16_ws_bytes((n, h, w, c), k, r, r, stride, pad, requested)
    assert ws_bytes > 0
    if requested:
        assert ws_bytes == wgrad_ws_bytes_host(shape, effective_splits(steps_of(shape), requested))
    ws_floats = E.floats_of(ws_bytes)
    label = "%s %s, %d splits requested:" % (name, regime, requested)
    wbuf, ws = guarded(ws_floats, guard=BAND)
    obuf, out = guarded(k * r * r * c, guard=BAND)
    dw, db = ops.conv2d_bwd_weight_bf16(dev["x"], dev["dy"], r, r, stride=stride, pad=pad, want_bias=True, splits=requested,
                                        out=out.view(k, r, r, c), ws=ws)
    assert dw.data_ptr() == out.data_ptr()
    E.verdict(label + " filter gradient", obuf, out, wbuf, ws_floats, dev["dw"])
    assert bool((db.double() == dev["db"]).all()), label + " the bias gradient is not the fp32 sum of the unrounded dy"
    ws.fill_(NAN)
    obuf, out = guarded(k * c_real * r * r, guard=BAND)
    bbuf, bias = guarded(k, guard=BAND)
    out.copy_(dev["before"].reshape(-1))
    bias.copy_(dev["before_b"])
    for _ in range(2):
        ops.conv2d_bwd_weight_acc_bf16(dev["x"], dev["dy"], r, r, out.view(k, c_real, r, r), bias, stride=stride, pad=pad,
                                       splits=requested, ws=ws)
    E.verdict(label + " gradient accumulated twice", obuf, out, wbuf, ws_floats, dev["acc"])
    E.verdict(label + " bias gradient accumulated twice", bbuf, bias, wbuf, ws_floats, dev["acc_b"])
    assert bool(operands_flag(dev)), label + " an operand's guard band changed"
    return 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(W_SHAPES))
def test_filter_gradient_every_regime_split_and_form(hip, name):
    """T1, T2, T3 x one request per effective split count of 1, 2, 3, 5, steps, steps + 1 x (plain + bias, accumulating twice
    + grad_b); layer3 and persistent: T1 with the library's own count (request 0)."""
    if name in W_ONCE:
        assert run_wgrad(name, "T1", 0) == 3
        return
    calls = sum(run_wgrad(name, regime, req) for regime in REGIMES for req in split_requests(W_SHAPES[name]))
    assert calls == 3 * len(REGIMES) * len(split_requests(W_SHAPES[name]))


@functools.lru_cache(maxsize=None)
def dgrad_on_device(name, regime):
    """Operands between bands; the filter goes through conv2d_transpose_filter and conv2d_pack_bf16 on the device, the words
    are checked against the host's flip, transposition and rounding, and copied between bands of the bf16 NaN word."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    ops_ = dgrad_case(name, regime)
    dev = {"bufs": [], "wbufs": [], "want": {}}
    for key in ("dy", "add", "act_y", "act_scale"):
        buf, dev[key] = guarded_copy(ops_[key])
        dev["bufs"].append((buf, ops_[key].numel()))
    words = ops.conv2d_pack_bf16(ops.conv2d_transpose_filter(ops_["w"].to(DEV)))
    assert torch.equal(words.cpu(), plane_bits(ops_["w"].flip(1, 2).permute(3, 1, 2, 0).contiguous())), "%s %s: the packed filter" % (name, regime)
    buf, dev["wq"] = guarded_words(words)
    dev["wbufs"].append((buf, words.numel()))
    return dev


def run_dgrad(name, regime, epilogue, label):
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k, r, stride, pad = D_SHAPES[name]
    dev = dgrad_on_device(name, regime)
    if epilogue not in dev["want"]:
        dev["want"][epilogue] = dgrad_case(name, regime)["want"][epilogue].to(DEV)
    ws_floats = E.floats_of(int(E.lib().frcnn_conv2d_bwd_data_bf16_ws_bytes(n, h, w, c, k, r, r, stride, pad)))
    assert (ws_floats > 0) == (stride > 1)
    wbuf, ws = guarded(ws_floats, guard=BAND)
    obuf, out = guarded(n * h * w * c, guard=BAND)
    got = ops.conv2d_bwd_data_bf16(dev["dy"], dev["wq"], (n, h, w, c), stride=stride, pad=pad,
                                   add=dev["add"] if epilogue != "none" else None,
                                   act_y=dev["act_y"] if epilogue in ("add_y", "add_y_scale") else None,
                                   act_scale=dev["act_scale"] if epilogue == "add_y_scale" else None, out=out.view(n, h, w, c), ws=ws)
    assert got.data_ptr() == out.data_ptr()
    label = "%s %s data gradient, %s epilogue %s" % (name, regime, label, epilogue)
    E.verdict(label, obuf, out, wbuf, ws_floats, dev["want"][epilogue])
    assert bool(operands_flag(dev)), label + ": an operand's guard band changed"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(D_SHAPES))
def test_data_gradient_every_regime_epilogue_tile_and_store_path(hip, name):
    """T1, T2, T3 x none / add / add + act_y / add + act_y + act_scale, under forced tiles 1 and 2 and store paths 0 and 64;
    layer3, dilate_stride and filter_stride under the library's tile and the default store path."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    runs = 0
    with hooks():
        for tile in (0,) if name in D_BIG else TILES:
            ops.set_conv_bf16_tile(tile)
            for algo in STORE_PATHS[:1] if name in D_BIG else STORE_PATHS:
                ops.set_conv_algo(algo)
                for regime in REGIMES:
                    for epilogue in EPILOGUES:
                        run_dgrad(name, regime, epilogue, "tile %d, algo %d," % (tile, algo))
                        runs += 1
    assert runs == len(REGIMES) * len(EPILOGUES) * (1 if name in D_BIG else len(TILES) * len(STORE_PATHS))


@pytest.mark.gpu
def test_k_48_is_refused_by_the_data_gradient(hip):
    """3x3s2_even of test_conv_f32_exact.py has k = 48: the forward kernel needs whole 32-channel K-steps, the wrapper and the
    library say so and dx stays untouched (3x3s2_even_k64 runs the same map)."""
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    n, h, w, c, k, r, stride, pad = E.SHAPES[REFUSED]
    ho, wo, m = geometry(E.SHAPES[REFUSED])
    dy = torch.zeros((n, ho, wo, k), dtype=torch.float32, device=DEV)
    packed = ops.conv2d_pack_bf16(torch.zeros((c, r, r, k), dtype=torch.float32, device=DEV))
    with pytest.raises(_hip.HipError):
        ops.conv2d_bwd_data_bf16(dy, packed, (n, h, w, c), stride=stride, pad=pad)
    ws = torch.empty(int(hip.frcnn_conv2d_bwd_data_bf16_ws_bytes(n, h, w, c, k, r, r, stride, pad)), dtype=torch.uint8, device=DEV)
    dx = torch.full((n, h, w, c), NAN, dtype=torch.float32, device=DEV)
    rc = hip.frcnn_conv2d_bwd_data_bf16(dy.data_ptr(), packed.data_ptr(), None, None, None, dx.data_ptr(), n, h, w, c, k, r, r,
                                        stride, pad, ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc != 0 and bool(torch.isnan(dx).all())


# ---- last: nothing is left set ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_hook_is_left_set(hip):
    """Tile mode 0 and algorithm 0: the settings' signature does not change when both are set to their defaults, and hook-free
    calls of both gradients still give float64."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    before = hip.frcnn_settings_signature()
    ops.set_conv_bf16_tile(0)
    ops.set_conv_algo(0)
    assert hip.frcnn_settings_signature() == before, "a bf16 convolution hook was left set"
    run_dgrad("3x3_odd_batch", "T2", "add_y_scale", "hook-free,")
    assert run_wgrad("3x3_odd_batch", "T2", 0) == 3
