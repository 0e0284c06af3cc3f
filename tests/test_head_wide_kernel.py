"""The wide detection tail (csrc/head.hip: head_wide_logits_kernel + head_wide_softmax_decode_kernel, entry points
frcnn_head_wide_softmax_decode[_lidar], ops.head_softmax_decode_wide) at the smallest shapes where it can go wrong.

  R      1, 31, 32 (one tile exactly), 33 (one row into a second tile), 37
  C      4 (one 16-byte chunk: the second half of the channel split is empty), 8 (one chunk per half), 252, 260 (halves
         of 128 + 124 and 132 + 128 channels: a ragged last stage, a second stage of one chunk), 2048 (8 stages per half)
  K      image 13, 21, 32, 81 -> 65 (one over two tiles), 105, 160 (five tiles exactly), 405 outputs;
         LiDAR 9, 11, 12 -> 72, 88, 96 (three tiles exactly) outputs
  sat    one class leads by 150: probability exactly 1, the others exactly 0, no NaN

What is asserted, and against what:
  1. integer operands in [-3, 3] (every partial sum an integer below 2^24 in any order, the method of
     tests/test_conv_f32_exact.py): cls_score / bbox_pred equal float64 with no tolerance; cls_prob / pred_boxes equal the
     float32 restatement (class-order softmax with a correctly rounded exp, decode32 / lidar_decode32 of
     tests/test_codec_head_kernels.py) bit for bit;
  2. on such operands at K <= 12 (image) / K <= 8 (LiDAR) all four outputs equal the fused kernel's, bit for bit;
  3. random operands (the generators of test_codec_head_kernels.head_case, fc7 drawn directly): the logits within the any-order
     fp32 summation bound (C + 2) 2^-24 (sum_c |fc7_c w_oc| + |b_o|) of float64 - C products and C + 1 additions, each rounded
     once, in whatever order: first-order gamma_(C+1), with one step of slack; cls_prob / pred_boxes bit-equal to the
     restatement applied to the kernel's OWN logits, and inside head_case's float64 bars evaluated on these shapes;
  4. rows 0..k of an R = 37 call equal an R = k + 1 call; a permutation of the RoIs permutes the outputs; two calls agree;
  5. outputs between NaN guard bands, pre-filled with NaN; every operand behind a NaN band and ending at the end of its
     allocation: bands intact, no NaN in any output;
  6. rejections: an error code and a message naming the entry point, the outputs keep their fill.
The unmarked tests hold a float32 restatement with numpy's own summation order to the same bars (a bar only one device's
rounding could meet fails without a GPU) and pin the header / exports.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_codec_head_kernels as T
from guarded_buffers import GUARD, guarded, guards_intact
from oracle import frcnn_oracle as O

DEV = "cuda:0"
f32 = np.float32
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCALE = T.HEAD_SCALE
NORM = T.HEAD_NORM
OUTPUTS = ("cls_score", "cls_prob", "bbox_pred", "pred_boxes")

# (form, R, C, K, variant): every R, C and K of the list above appears for both forms
CASES = [
    ("image", 1, 4, 13, "normal"), ("image", 31, 8, 21, "normal"), ("image", 32, 252, 32, "normal"),
    ("image", 33, 260, 81, "normal"), ("image", 37, 2048, 21, "normal"), ("image", 37, 2048, 81, "normal"),
    ("image", 37, 260, 13, "sat"),
    ("lidar", 1, 8, 9, "normal"), ("lidar", 31, 4, 11, "normal"), ("lidar", 32, 260, 12, "normal"),
    ("lidar", 33, 252, 9, "normal"), ("lidar", 37, 2048, 12, "normal"), ("lidar", 37, 2048, 11, "normal"),
]
# the fused kernel's range, for the cross-check
SMALL_CASES = [("image", 37, 260, 12, "normal"), ("image", 33, 2048, 2, "normal"), ("image", 1, 4, 5, "normal"),
               ("lidar", 37, 252, 8, "normal"), ("lidar", 32, 8, 4, "normal"), ("lidar", 33, 2048, 2, "normal")]


def _id(c):
    return "%s-R%d-C%d-K%d-%s" % c


def _elems(form):
    return 4 if form == "image" else 7


def _boxes_and_anchors(r_, g):
    rois = torch.cat((torch.zeros(r_, 1), T._plain_boxes(r_, 4, g, 4.0, 600.0)), 1).contiguous()
    return rois, T._anchors3d(r_, g)


@functools.lru_cache(maxsize=None)
def integer_case(case):
    """fc7, weights in [-3, 3], biases in [-5, 5], all integers held in float32."""
    form, r_, c_, k, _ = case
    e = _elems(form)
    g = torch.Generator().manual_seed(9100 + 7 * r_ + c_ + 31 * k + e)
    ri = lambda *shape, lim=3: torch.randint(-lim, lim + 1, shape, generator=g).float()
    rois, anc = _boxes_and_anchors(r_, g)
    return dict(fc7=ri(r_, c_), wc=ri(k, c_), bc=ri(k, lim=5), wb=ri(e * k, c_), bb=ri(e * k, lim=5), rois=rois,
                anchors=anc if e == 7 else None, stds=NORM[form][0], means=NORM[form][1])


@functools.lru_cache(maxsize=None)
def random_case(case):
    """head_case of tests/test_codec_head_kernels.py with fc7 drawn directly (P = 1): (inputs, float64 reference, bars)."""
    form, r_, c_, k, variant = case
    e = _elems(form)
    g = torch.Generator().manual_seed(9500 + CASES.index(case))
    fc7 = torch.randn(r_, c_, generator=g) + 0.3
    sc = 1.0 / np.sqrt(c_)
    wc, bc = torch.randn(k, c_, generator=g) * sc, torch.randn(k, generator=g) * 0.5
    wb, bb = torch.randn(e * k, c_, generator=g) * sc, torch.randn(e * k, generator=g) * 0.1
    if variant == "sat":
        bc[1] += 150.0
    rois, anc = _boxes_and_anchors(r_, g)
    stds, means = NORM[form]
    inp = dict(fc7=fc7, wc=wc, bc=bc, wb=wb, bb=bb, rois=rois, anchors=anc if e == 7 else None, stds=stds, means=means)
    f64 = fc7.double()
    score = F.linear(f64, wc.double(), bc.double())
    prob = F.softmax(score, 1)
    raw = F.linear(f64, wb.double(), bb.double())
    d = (raw.view(r_, k, e) * torch.tensor(stds, dtype=torch.float64) + torch.tensor(means, dtype=torch.float64)).view(r_, -1)
    b = rois[:, 1:5].double()
    bs = b / SCALE
    if e == 4:
        boxes = O.bbox_transform_inv(b, d, SCALE)
        dbar = T._decode_bar(boxes, 4)
    else:
        boxes = O.lidar_3d_bbox_transform_inv(b, anc.double(), d, SCALE)
        centre = torch.stack((bs[:, 0] + (bs[:, 2] - bs[:, 0] + 1) / 2, bs[:, 1] + (bs[:, 3] - bs[:, 1] + 1) / 2,
                              anc[:, 2].double()) + (torch.zeros(r_, dtype=torch.float64),) * 4, 1).numpy()
        dbar = T._decode_bar(boxes, 7, centre)
    ref = dict(cls_score=score, cls_prob=prob, bbox_pred=raw, pred_boxes=boxes)
    big = lambda t_: max(1.0, float(t_.abs().max()))
    bars = dict(cls_score=1e-5 * big(score), cls_prob=1e-5, bbox_pred=1e-5 * big(raw))
    ln, wd = bs[:, 2] - bs[:, 0] + 1, bs[:, 3] - bs[:, 1] + 1
    diag = torch.sqrt(ln * ln + wd * wd).view(-1, 1, 1)
    std = torch.tensor(stds, dtype=torch.float64).view(1, 1, e)
    bx = boxes.view(r_, k, e)
    if e == 4:
        half = torch.stack(((bx[..., 2] - bx[..., 0]) / 2, (bx[..., 3] - bx[..., 1]) / 2) * 2, 2).abs()
        move = std[..., [0, 1, 0, 1]] * diag + std[..., [2, 3, 2, 3]] * half
    else:
        ht = anc[:, 5].double().view(-1, 1, 1)
        move = torch.cat((std[..., 0:2] * diag.expand(r_, k, 2), (std[..., 2:3] * ht).expand(r_, k, 1),
                          std[..., 3:6] * bx[..., 3:6].abs(), std[..., 6:7].expand(r_, k, 1)), 2)
    bars["pred_boxes"] = dbar + bars["bbox_pred"] * move.reshape(r_, -1).numpy()
    # any-order fp32 summation bound of the two Linear layers
    a64 = f64.abs()
    sum_bound = lambda w_, b_: ((c_ + 2) * 2.0 ** -24 * (a64 @ w_.double().abs().t() + b_.double().abs())).numpy()
    bounds = dict(cls_score=sum_bound(wc, bc), bbox_pred=sum_bound(wb, bb))
    return inp, ref, bars, bounds


@T._quiet
def tail32(score, raw, rois, anchors, stds, means, scale):
    """Softmax and decode of both tail kernels on given float32 logits: maximum, exp32(s - m), the sum in class order, a
    divide; raw * std + mean through decode32 / lidar_decode32."""
    score, raw = np.asarray(score, f32), np.asarray(raw, f32)
    r_, k = score.shape
    e = raw.shape[1] // k
    m = score.max(1, keepdims=True)
    ex = T.exp32(score - m)
    s = np.zeros((r_, 1), f32)
    for q in range(k):
        s = s + ex[:, q:q + 1]
    prob = ex / s
    d = raw.reshape(r_, k, e) * np.asarray(stds, f32) + np.asarray(means, f32)
    if e == 4:
        boxes = T.decode32(rois[:, 1:5], d.reshape(r_, -1), scale)
    else:
        boxes = T.lidar_decode32(rois[:, 1:5], anchors, d.reshape(r_, -1), scale)
    return prob, boxes


def _tail32_of(inp, score, raw):
    return tail32(score, raw, T._np(inp["rois"]), None if inp["anchors"] is None else T._np(inp["anchors"]),
                  inp["stds"], inp["means"], SCALE)


def _run(inp, rows=None):
    """ops.head_softmax_decode_wide on the case's operands (optionally on a selection of its RoIs)."""
    sel = (lambda t_: t_) if rows is None else (lambda t_: t_[rows].contiguous())
    anc = inp["anchors"]
    out = T._ops().head_softmax_decode_wide(
        sel(inp["fc7"]).to(DEV), inp["wc"].to(DEV), inp["bc"].to(DEV), inp["wb"].to(DEV), inp["bb"].to(DEV),
        sel(inp["rois"]).to(DEV), list(inp["stds"]), list(inp["means"]), SCALE,
        roi_anchors_3d=None if anc is None else sel(anc).to(DEV))
    return {n: T._np(out[n]) for n in OUTPUTS}


def _linear64(inp):
    f64 = inp["fc7"].double()
    return (F.linear(f64, inp["wc"].double(), inp["bc"].double()).numpy(),
            F.linear(f64, inp["wb"].double(), inp["bb"].double()).numpy())


# ================================================================================================
# without a GPU
# ================================================================================================
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cpu_restatement_wide(case):
    """float32 logits in numpy's summation order, then tail32: inside the bounds and bars the device is held to."""
    inp, ref, bars, bounds = random_case(case)
    fc7 = T._np(inp["fc7"])
    score = fc7 @ T._np(inp["wc"]).T + T._np(inp["bc"])
    raw = fc7 @ T._np(inp["wb"]).T + T._np(inp["bb"])
    prob, boxes = _tail32_of(inp, score, raw)
    got = dict(cls_score=score, cls_prob=prob, bbox_pred=raw, pred_boxes=boxes)
    for name in ("cls_score", "bbox_pred"):
        T._assert_close("head_wide", _id(case), name + " vs the summation bound", got[name], ref[name], bounds[name], "cpu")
    for name in OUTPUTS:
        T._assert_close("head_wide", _id(case), name, got[name], ref[name], bars[name], "cpu")
    if case[4] == "sat":
        assert (prob[:, 1] == 1).all() and (np.delete(prob, 1, 1) == 0).all()
        assert (T._np(ref["cls_prob"]).astype(f32)[:, 1] == 1).all()


@pytest.mark.parametrize("case", CASES + SMALL_CASES, ids=_id)
def test_integer_operands_are_exact_in_any_order(case):
    """The premise of the exact tests: sum_c |fc7 w| + |b| stays below 2^24, so every partial sum is an exact integer."""
    inp = integer_case(case)
    for w_, b_ in ((inp["wc"], inp["bc"]), (inp["wb"], inp["bb"])):
        worst = float((inp["fc7"].double().abs() @ w_.double().abs().t() + b_.double().abs()).max())
        assert worst < 2 ** 24 and worst <= 9 * case[2] + 5


def test_header_declares_and_library_exports_the_wide_entry_points():
    from faster_rcnn_pytorch_multimodal_amd import _hip
    with open(os.path.join(ROOT, "include", "frcnn_hip.h")) as fh:
        header = fh.read()
    lib = _hip.load()
    for name in ("frcnn_head_wide_softmax_decode", "frcnn_head_wide_softmax_decode_lidar"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _hip.PROTOTYPES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert lib.frcnn_version() >= 123


# ================================================================================================
# on the device
# ================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_wide_exact_on_integer_operands(hip, case):
    inp = integer_case(case)
    got = _run(inp)
    score64, raw64 = _linear64(inp)
    assert np.array_equal(got["cls_score"].astype(np.float64), score64), "cls_score differs from float64"
    assert np.array_equal(got["bbox_pred"].astype(np.float64), raw64), "bbox_pred differs from float64"
    prob, boxes = _tail32_of(inp, score64.astype(f32), raw64.astype(f32))
    T._assert_bits("head_wide", _id(case), "cls_prob", got["cls_prob"], prob)
    T._assert_bits("head_wide", _id(case), "pred_boxes", got["pred_boxes"], boxes)
    assert not np.isnan(got["cls_prob"]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", SMALL_CASES, ids=_id)
def test_wide_equals_fused_kernel_on_integer_operands(hip, case):
    inp = integer_case(case)
    got = _run(inp)
    r_, c_ = inp["fc7"].shape
    anc = inp["anchors"]
    fused = T._ops().head_fc_softmax_decode(
        inp["fc7"].view(r_, 1, 1, c_).to(DEV), inp["wc"].to(DEV), inp["bc"].to(DEV), inp["wb"].to(DEV), inp["bb"].to(DEV),
        inp["rois"].to(DEV), list(inp["stds"]), list(inp["means"]), SCALE, roi_anchors_3d=None if anc is None else anc.to(DEV))
    for name in OUTPUTS:
        T._assert_bits("head_wide", _id(case), name + " vs the fused kernel", got[name], T._np(fused[name]))
    score64, raw64 = _linear64(inp)
    assert np.array_equal(got["cls_score"].astype(np.float64), score64)
    assert np.array_equal(got["bbox_pred"].astype(np.float64), raw64)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_wide_random_operands(hip, case):
    inp, ref, bars, bounds = random_case(case)
    got = _run(inp)
    for name in ("cls_score", "bbox_pred"):
        T._assert_close("head_wide", _id(case), name + " vs the summation bound", got[name], ref[name], bounds[name], "gpu")
    prob, boxes = _tail32_of(inp, got["cls_score"], got["bbox_pred"])
    T._assert_bits("head_wide", _id(case), "cls_prob vs softmax of own cls_score", got["cls_prob"], prob)
    T._assert_bits("head_wide", _id(case), "pred_boxes vs decode of own bbox_pred", got["pred_boxes"], boxes)
    for name in OUTPUTS:
        T._assert_close("head_wide", _id(case), name, got[name], ref[name], bars[name], "gpu")
    if case[4] == "sat":
        p = got["cls_prob"]
        assert (p[:, 1] == 1).all() and (np.delete(p, 1, 1) == 0).all() and not np.isnan(p).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[4], CASES[3], CASES[12], CASES[10]], ids=_id)
def test_wide_rows_are_independent_and_runs_repeat(hip, case):
    inp = random_case(case)[0]
    r_ = case[1]
    full = _run(inp)
    again = _run(inp)
    for name in OUTPUTS:
        T._assert_bits("head_wide", _id(case), name + " second call", again[name], full[name])
    for k in sorted({0, 30, 31, 32, r_ - 2} & set(range(r_))):          # R = k + 1: 1, 31, 32 (one tile), 33
        part = _run(inp, rows=torch.arange(k + 1))
        for name in OUTPUTS:
            T._assert_bits("head_wide", _id(case), "%s rows 0..%d alone" % (name, k), part[name], full[name][:k + 1])
    perm = torch.randperm(r_, generator=torch.Generator().manual_seed(3))
    assert not torch.equal(perm, torch.arange(r_))
    moved = _run(inp, rows=perm)
    for name in OUTPUTS:
        T._assert_bits("head_wide", _id(case), name + " permuted RoIs", moved[name], full[name][perm.numpy()])


def _at_end(t_, pad=GUARD):
    """A device copy of ``t_`` that ends where its allocation ends, behind ``pad`` floats of NaN (pad * 4 bytes keeps the
    16-byte alignment): a read in front of the operand brings a NaN into the outputs."""
    if t_ is None:
        return None, None
    buf = torch.full((pad + t_.numel(),), float("nan"), dtype=torch.float32, device=DEV)
    buf[pad:] = t_.reshape(-1).to(DEV)
    return buf, buf[pad:].view(t_.shape)


def _abi_call(lib, form, ptrs, r_, c_, k, stds, means, scale=SCALE):
    H = T._hip()
    head = [ptrs["fc7"], r_, c_, ptrs["wc"], ptrs["bc"], ptrs["wb"], ptrs["bb"], k, ptrs["rois"]]
    tail = [H.float_array(stds), H.float_array(means), scale] + [ptrs[n] for n in OUTPUTS] + [
        torch.cuda.current_stream().cuda_stream]
    if form == "image":
        rc = lib.frcnn_head_wide_softmax_decode(*(head + tail))
    else:
        rc = lib.frcnn_head_wide_softmax_decode_lidar(*(head + [ptrs["anchors"]] + tail))
    torch.cuda.synchronize()
    return rc


def _out_sizes(form, r_, k):
    e = _elems(form)
    return dict(cls_score=r_ * k, cls_prob=r_ * k, bbox_pred=r_ * e * k, pred_boxes=r_ * e * k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5], CASES[7], CASES[9], CASES[12]], ids=_id)
def test_wide_inside_guard_bands(hip, case):
    form, r_, c_, k, _ = case
    inp = random_case(case)[0]
    held = {n: _at_end(inp[n]) for n in ("fc7", "wc", "bc", "wb", "bb", "rois", "anchors")}
    sizes = _out_sizes(form, r_, k)
    outs = {n: guarded(sizes[n]) for n in OUTPUTS}
    ptrs = {n: (None if v[1] is None else v[1].data_ptr()) for n, v in held.items()}
    ptrs.update({n: outs[n][1].data_ptr() for n in OUTPUTS})
    rc = _abi_call(hip, form, ptrs, r_, c_, k, inp["stds"], inp["means"])
    assert rc == 0, hip.frcnn_last_error()
    want = _run(inp)
    for n in OUTPUTS:
        assert guards_intact(outs[n][0], sizes[n]), "%s: a store outside the output" % n
        assert not bool(torch.isnan(outs[n][1]).any()), "%s: an element not written, or a read outside an operand" % n
        T._assert_bits("head_wide", _id(case), n + " in guarded buffers", outs[n][1].view(want[n].shape), want[n])
    for n, (buf, view) in held.items():
        if buf is not None:
            assert bool(torch.isnan(buf[:GUARD]).all()) and torch.equal(view.cpu(), inp[n]), "%s was written to" % n


REJECTS = [(form, what) for form in ("image", "lidar") for what in
           ("null fc7", "null w_box", "null b_cls", "null rois", "null pred_boxes", "null stds", "c%4", "k<2", "r=0", "r<0",
            "scale=0", "unaligned w_cls", "aliased outputs")] + [("lidar", "null anchors")]


@pytest.mark.gpu
@pytest.mark.parametrize("rej", REJECTS, ids=lambda r: "%s-%s" % r)
def test_wide_rejections(hip, rej):
    """An error code, a message that names the entry point, nothing launched: the outputs keep their fill."""
    form, what = rej
    e = _elems(form)
    r_, c_, k = 2, 6 if what == "c%4" else 8, 1 if what == "k<2" else 3
    g = torch.Generator().manual_seed(5)
    dev = dict(fc7=torch.randn(r_, c_, generator=g), wc=torch.randn(k + 1, c_, generator=g), bc=torch.zeros(k),
               wb=torch.randn(e * k, c_, generator=g), bb=torch.zeros(e * k), rois=torch.tensor([[0.0, 1.0, 2.0, 30.0, 40.0]] * r_),
               anchors=T._anchors3d(r_, g) if e == 7 else None)
    dev = {n: (None if v is None else v.to(DEV).contiguous()) for n, v in dev.items()}
    sizes = _out_sizes(form, r_, max(k, 2))
    outs = {n: torch.full((sizes[n],), -7.0, device=DEV) for n in OUTPUTS}
    ptrs = {n: (None if v is None else v.data_ptr()) for n, v in dev.items()}
    ptrs.update({n: outs[n].data_ptr() for n in OUTPUTS})
    stds, means, scale, rows = NORM[form][0], NORM[form][1], SCALE, r_
    if what.startswith("null ") and what != "null stds":
        ptrs[{"w_box": "wb", "b_cls": "bc"}.get(what[5:], what[5:])] = None
    elif what == "r=0":
        rows = 0
    elif what == "r<0":
        rows = -1
    elif what == "scale=0":
        scale = 0.0
    elif what == "unaligned w_cls":
        ptrs["wc"] += 4                                              # one float on: (K, C) still lies inside (K + 1, C)
    elif what == "aliased outputs":
        ptrs["pred_boxes"] = ptrs["bbox_pred"]                       # the second launch's outputs are the first one's scratch
    if what == "null stds":
        H = T._hip()
        head = [ptrs["fc7"], rows, c_, ptrs["wc"], ptrs["bc"], ptrs["wb"], ptrs["bb"], k, ptrs["rois"]]
        tail = [None, H.float_array(means), scale] + [ptrs[n] for n in OUTPUTS] + [torch.cuda.current_stream().cuda_stream]
        rc = (hip.frcnn_head_wide_softmax_decode(*(head + tail)) if e == 4 else
              hip.frcnn_head_wide_softmax_decode_lidar(*(head + [ptrs["anchors"]] + tail)))
        torch.cuda.synchronize()
    else:
        rc = _abi_call(hip, form, ptrs, rows, c_, k, stds, means, scale)
    msg = (hip.frcnn_last_error() or b"").decode()
    assert rc != 0 and "head_wide_softmax_decode" in msg, (rc, msg)
    for n in OUTPUTS:
        assert bool((outs[n] == -7.0).all()), n


@pytest.mark.gpu
def test_wide_ops_wrapper_rejects_inconsistent_operands(hip):
    ops, H = T._ops(), T._hip()
    inp = integer_case(CASES[0])
    args = lambda **kw: dict(dict(fc7=inp["fc7"].to(DEV), w_cls=inp["wc"].to(DEV), b_cls=inp["bc"].to(DEV), w_box=inp["wb"].to(DEV),
                                  b_box=inp["bb"].to(DEV), rois=inp["rois"].to(DEV), stds=list(inp["stds"]),
                                  means=list(inp["means"]), scale=SCALE), **kw)
    with pytest.raises(H.HipError, match="head_softmax_decode_wide"):
        ops.head_softmax_decode_wide(**args(w_box=inp["wb"][:-1].contiguous().to(DEV)))
    with pytest.raises(H.HipError, match="head_softmax_decode_wide"):
        ops.head_softmax_decode_wide(**args(fc7=inp["fc7"].view(1, 1, 1, -1).to(DEV)))
    with pytest.raises(H.HipError, match="head_softmax_decode_wide"):
        ops.head_softmax_decode_wide(**args(roi_anchors_3d=torch.zeros(1, 7, device=DEV)))   # 4-DoF weights, LiDAR call
    with pytest.raises(H.HipError, match="MI355X"):
        ops.head_softmax_decode_wide(**args(fc7=inp["fc7"]))
