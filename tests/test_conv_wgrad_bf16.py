"""The bf16-operand filter gradient (conv_wgrad_bf16: frcnn_conv2d_bwd_weight_bf16 / _acc_bf16) through ``ops``, against
float64 on the host.

    dw[k][r][s][c] = sum over output pixels m of  bf16(dy)[m][k] * bf16(x)[pixel of m under tap (r, s)][c],  fp32 accumulation

Shapes (N,H,W,C,K, filter): the smallest at which the 128 x 128 tile, the 32-pixel reduction step and the pixel split can go
wrong, and one real layer3 shape.  Every shape runs with 1, 2 and 3 pixel splits and with one more than it has reduction steps
(clamped to them: one step per slab).
  * integer operands in [-3, 3]: bf16 holds them, every partial sum is an integer below 2^24 - the result equals float64 bit for bit;
  * normal operands against float64 on the bf16-ROUNDED operands: within n * 2^-24 * sum|products| per element, the fp32
    accumulation bound with n = the number of accumulated terms (the output pixels);
  * normal operands against float64 on the UNROUNDED operands: within 2^-7 * sum|products| (two roundings of 2^-8 each, plus
    the accumulation term, which is of second order here) - and NOT equal to it: the rounding is really there;
  * the accumulating form adds to a non-zero gradient, and again on a second call;
  * two runs are bit-equal; NaN guard bands around the output and around the workspace (slabs and bias partials) are intact, and
    every element of the output is written.
"""
import pytest

from guarded_buffers import DEV, GUARD, guarded, guards_intact

# name -> (n, h, w, c, k, r, stride, pad)
SHAPES = {
    "tail3_k32": (1, 5, 7, 32, 32, 3, 1, 1),          # 35 pixels: one full reduction step and a tail of 3; K below the tile edge
    "k96_1x1": (1, 6, 6, 64, 96, 1, 1, 0),            # K is one and a half tiles
    "strided3x3": (1, 9, 11, 32, 64, 3, 2, 1),        # the strided form
    "batch_1x1s2": (2, 4, 4, 96, 32, 1, 2, 0),        # a batch boundary inside a reduction step
    "layer3_3x3": (1, 38, 63, 256, 256, 3, 1, 1),     # one real layer3 shape
}
_CACHE = {}


def out_hw(h, w, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1


def steps_of(name):
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = out_hw(h, w, r, stride, pad)
    return (n * ho * wo + 31) // 32


def split_counts(name):
    return (1, 2, 3, steps_of(name) + 1)


def rbf16(t):
    import torch
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def operands(name, kind):
    """(x (n,h,w,c), dy (n,ho,wo,k)) as float64 host tensors holding fp32 values."""
    import torch
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = out_hw(h, w, r, stride, pad)
    gen = torch.Generator().manual_seed(sorted(SHAPES).index(name) * 7 + (1 if kind == "int" else 2))
    if kind == "int":
        x = torch.randint(-3, 4, (n, h, w, c), generator=gen).double()
        dy = torch.randint(-3, 4, (n, ho, wo, k), generator=gen).double()
    else:
        x = torch.randn((n, h, w, c), generator=gen, dtype=torch.float32).double()
        dy = torch.randn((n, ho, wo, k), generator=gen, dtype=torch.float32).double()
    return x, dy


def dw_float64(name, x, dy):
    """The definition in float64: (k, r, s, c)."""
    import torch
    import torch.nn.functional as F
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    cols = F.unfold(x.permute(0, 3, 1, 2), (r, r), padding=pad, stride=stride)             # (n, c*r*r, L)
    cols = cols.reshape(n, c, r, r, -1).permute(0, 4, 2, 3, 1).reshape(-1, r * r * c)      # (M, (r, s, c))
    return (dy.reshape(-1, k).t() @ cols).reshape(k, r, r, c)


def reference(name, kind):
    """Computed once per (shape, kind) and left unchanged: the operands, float64 on them as given (``exact``), on the rounded
    operands (``rounded``) and the sums of |products| of each."""
    if (name, kind) not in _CACHE:
        x, dy = operands(name, kind)
        ref = {"x": x, "dy": dy, "exact": dw_float64(name, x, dy)}
        if kind != "int":
            ref["abs"] = dw_float64(name, x.abs(), dy.abs())
            ref["rounded"] = dw_float64(name, rbf16(x), rbf16(dy))
            ref["abs_rounded"] = dw_float64(name, rbf16(x).abs(), rbf16(dy).abs())
        _CACHE[(name, kind)] = ref
    return _CACHE[(name, kind)]


# ---- guarded device runs (guarded / guards_intact: guarded_buffers.py) -----------------------------------------------------------
def run_device(name, x, dy, splits, before=None, want_bias=False):
    """One guarded launch.  ``before`` None: frcnn_conv2d_bwd_weight_bf16 into a NaN-filled dw (k,r,s,c); else the accumulating
    form into a (k,c,r,s) gradient that holds ``before``.  Returns (result as float64 host tensor, db or None)."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    xd, dyd = x.float().to(DEV), dy.float().to(DEV)
    ws_bytes = ops.conv2d_bwd_weight_bf16_ws_bytes((n, h, w, c), k, r, r, stride, pad, splits)
    ws_floats = max((ws_bytes + 3) // 4, 4)
    wbuf, ws = guarded(ws_floats)
    obuf, out = guarded(k * r * r * c)
    db = None
    if before is None:
        res, db = ops.conv2d_bwd_weight_bf16(xd, dyd, r, r, stride=stride, pad=pad, want_bias=want_bias, splits=splits,
                                             out=out.view(k, r, r, c), ws=ws)
        assert res.data_ptr() == out.data_ptr()
    else:
        out.copy_(before.float().reshape(-1))
        gb = torch.zeros(k, dtype=torch.float32, device=DEV) if want_bias else None
        ops.conv2d_bwd_weight_acc_bf16(xd, dyd, r, r, out.view(k, c, r, r), gb, stride=stride, pad=pad, splits=splits, ws=ws)
        ops.conv2d_bwd_weight_acc_bf16(xd, dyd, r, r, out.view(k, c, r, r), gb, stride=stride, pad=pad, splits=splits, ws=ws)
        db = gb
    torch.cuda.synchronize()
    assert guards_intact(obuf, out.numel()), "%s: wrote outside the output" % name
    assert guards_intact(wbuf, ws_floats), "%s: wrote outside the workspace" % name
    host = out.cpu().double()
    assert not torch.isnan(host).any(), "%s: an output element was not written" % name
    return host.view((k, r, r, c) if before is None else (k, c, r, r)), (db.cpu().double() if db is not None else None)


CASES = [(name, sp) for name in SHAPES for sp in split_counts(name)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,splits", CASES, ids=["%s-z%d" % c for c in CASES])
def test_integer_operands_are_exact(hip, name, splits):
    import torch
    ref = reference(name, "int")
    got, db = run_device(name, ref["x"], ref["dy"], splits, want_bias=True)
    assert torch.equal(got, ref["exact"])
    assert torch.equal(db, ref["dy"].reshape(-1, ref["dy"].shape[-1]).sum(0))


@pytest.mark.gpu
@pytest.mark.parametrize("name,splits", CASES, ids=["%s-z%d" % c for c in CASES])
def test_normal_operands_within_the_bounds(hip, name, splits):
    import torch
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = out_hw(h, w, r, stride, pad)
    terms = n * ho * wo
    ref = reference(name, "normal")
    got, _ = run_device(name, ref["x"], ref["dy"], splits)
    again, _ = run_device(name, ref["x"], ref["dy"], splits)
    assert torch.equal(got, again), "two runs differ"
    err_r = (got - ref["rounded"]).abs()
    bound_r = terms * 2.0 ** -24 * ref["abs_rounded"]
    err_u = (got - ref["exact"]).abs()
    bound_u = 2.0 ** -7 * ref["abs"]
    print("%s z=%d: max err/bound against rounded operands %.3g, against unrounded operands %.3g"
          % (name, splits, float((err_r / bound_r.clamp_min(1e-300)).max()), float((err_u / bound_u.clamp_min(1e-300)).max())))
    assert bool((err_r <= bound_r).all())
    assert bool((err_u <= bound_u).all())
    assert not torch.equal(got, ref["exact"].float().double()), "no rounding of the operands visible"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("splits", (1, 3))
def test_accumulating_form_adds_twice(hip, name, splits):
    """grad (k,c,r,s) = before + 2 * dw on integer operands: exact, whatever the order of the additions."""
    import torch
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ref = reference(name, "int")
    gen = torch.Generator().manual_seed(99)
    before = torch.randint(-5, 6, (k, c, r, r), generator=gen).double()
    got, db = run_device(name, ref["x"], ref["dy"], splits, before=before, want_bias=True)
    assert torch.equal(got, before + 2.0 * ref["exact"].permute(0, 3, 1, 2))
    assert torch.equal(db, 2.0 * ref["dy"].reshape(-1, k).sum(0))


@pytest.mark.gpu
def test_library_chooses_the_split_count_and_rejects_a_negative_one(hip):
    """splits = 0 lets the library choose (same bound); a negative count raises."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    name = "strided3x3"
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ref = reference(name, "normal")
    xd, dyd = ref["x"].float().to(DEV), ref["dy"].float().to(DEV)
    auto = ops.conv2d_bwd_weight_bf16(xd, dyd, r, r, stride=stride, pad=pad)[0].cpu().double()
    ho, wo = out_hw(h, w, r, stride, pad)
    assert bool(((auto - ref["rounded"]).abs() <= n * ho * wo * 2.0 ** -24 * ref["abs_rounded"]).all())
    with pytest.raises(Exception):
        ops.conv2d_bwd_weight_bf16(xd, dyd, r, r, stride=stride, pad=pad, splits=-1)


def test_an_oversized_split_count_is_refused():
    """A caller's split count is taken as given up to 256 MB of slabs (and 65535 launches in z): beyond, the workspace query
    answers 0 and the call FRCNN_ERR_ARG, instead of a launch that cannot run.  No GPU needed: the query is host code."""
    from faster_rcnn_pytorch_multimodal_amd import _hip
    lib = _hip.load()
    shape = (1, 150, 250, 256, 256, 3, 3, 1, 1)                # 1172 steps, 2.36 MB per slab
    assert lib.frcnn_conv2d_bwd_weight_bf16_ws_bytes(*shape, 100) >= 98 * 256 * 2304 * 4       # 12 steps per slab: 98 slabs, 231 MB
    assert lib.frcnn_conv2d_bwd_weight_bf16_ws_bytes(*shape, 200) == 0                          # 196 slabs, 462 MB
    assert lib.frcnn_conv2d_bwd_weight_bf16_ws_bytes(*shape, 0) > 0
