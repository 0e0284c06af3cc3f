"""The loss, statistics and small training kernels (csrc/train_ops.hip, fpn_level_map of csrc/boxes.hip) at their
edges, each called directly through ops.py and compared with a float64 CPU reference built from the oracle's own
functions (O.smooth_l1_loss, O.huber_loss, F.cross_entropy, O.compute_bbox_var, O.categorical_entropy,
O.categorical_mutual_information, O.bayesian_cross_entropy, O.fpn_level_map) and torch autograd.

Case builders return (inputs, float64 reference, bars).  The GPU tests (marked gpu) run the kernel against them; the
unmarked ``test_cpu_restatement_*`` tests restate each kernel's arithmetic in float32 torch on the CPU and require the
same bar with 4x headroom, so a bar that only one device's rounding could meet, or inputs on which the reference itself
is unstable, fail without a GPU.

Which case reaches which regime (case ids as pytest prints them):
  rpn_loss block partition   hw3-A5-ld30 (total 15 < 256: per = 1, most blocks empty), hw204-A25-ld152 (per = 20),
                             hw211-A9-ld56 (per = 8, ragged last block, ld % 4 != 0), hw4400-A15-ld96 (total 66000,
                             per = 258: second trip of the stride loop)
  rpn_loss ld == 6A          hw3-A5-ld30 (no padding memset)
  no labelled anchor         *-none_labelled (cnt > 0 guards), det *-no_fg
  det_loss R / K / E         R1 R255 R257 R4096 x K4, K2 K9 x R257, forms plain4 lidar7 alea4 alea7; R = 4097 rejected
  extreme finite logits      *-wide (log-sum-exp max subtraction)
  Huber breakpoints          *-breakpoints (|diff| in {0, .5, 1, 1.5} exactly)
  bayes_ce                   N300-K16-S20 (KMAX), K = 17 rejected, *-var (variance exactly 0), N257 / N300 (N % 256 != 0)
  grid-stride second trip    dropout big, mc_* / exp n = 8192*256+77, spatial_mean_bwd (300,7,2048), act_bwd big
  fpn_level_map              level-boundary squares, s x (s+-1), 895 x 897 (only `+ eps` lifts it to level 6), zero /
                             negative area, 1x1, 4000x4000

Bars.  Where the existing suite has one it is used: 1e-5 on O(1) losses, 1e-6 on drpn, 1e-7 on dcls / dbox (tests/
test_gpu_parity.py), 2e-5 / 2e-6 / 5e-6 on the Bayesian cross entropy (tests/test_uncertainty.py), each multiplied by
max(1, max |per-element term of the float64 reference|).  The others are derived from fp32 rounding next to the case.
A bar the float32 restatement could not meet with 4x headroom is listed in WIDENED with the measured error.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import frcnn_oracle as O

DEV = "cuda:0"
U = 2.0 ** -23                       # fp32 machine epsilon (spacing of floats in [1, 2))
GRID_CAP = 8192 * 256                # elementwise kernels launch min(ceil(n / 256), 8192) blocks of 256 and stride
BIG = GRID_CAP + 77
HEADROOM = 4.0

# (section, case id, tensor) -> (bar, error of the float32 CPU restatement that made the default bar too tight).  The bar is
# 4x that error, rounded up to three digits.  All of them are det_loss gradients that are O(1) or larger (R = 1, where
# 1 / R does not shrink them, and exp(8) of the aleatoric extremes), where 1e-7 is below fp32's own rounding.
WIDENED = {
    ("det", "R1-K4-plain4-normal", "dcls"): (1.04e-07, 2.578e-08),
    ("det", "R1-K4-plain4-normal", "dbox"): (1.91e-07, 4.768e-08),
    ("det", "R1-K4-plain4-wide", "dbox"): (1.91e-07, 4.768e-08),
    ("det", "R1-K4-plain4-no_fg", "dcls"): (1.24e-07, 3.100e-08),
    ("det", "R1-K4-plain4-breakpoints", "dcls"): (2.07e-07, 5.167e-08),
    ("det", "R1-K4-plain4-breakpoints", "dbox"): (1.91e-07, 4.768e-08),
    ("det", "R1-K4-lidar7-normal", "dcls"): (1.04e-07, 2.578e-08),
    ("det", "R1-K4-lidar7-normal", "dbox"): (1.53e-06, 3.815e-07),
    ("det", "R1-K4-lidar7-wide", "dbox"): (1.53e-06, 3.815e-07),
    ("det", "R1-K4-lidar7-no_fg", "dcls"): (1.24e-07, 3.100e-08),
    ("det", "R1-K4-lidar7-breakpoints", "dcls"): (2.07e-07, 5.167e-08),
    ("det", "R1-K4-lidar7-breakpoints", "dbox"): (1.53e-06, 3.815e-07),
    ("det", "R1-K4-alea4-normal", "dcls"): (1.04e-07, 2.578e-08),
    ("det", "R1-K4-alea4-normal", "dbox"): (1.13e-06, 2.805e-07),
    ("det", "R1-K4-alea4-normal", "dvar"): (7.34e-07, 1.835e-07),
    ("det", "R1-K4-alea4-wide", "dvar"): (4.90e-07, 1.223e-07),
    ("det", "R1-K4-alea4-no_fg", "dcls"): (1.24e-07, 3.100e-08),
    ("det", "R1-K4-alea4-breakpoints", "dcls"): (2.07e-07, 5.167e-08),
    ("det", "R1-K4-alea4-breakpoints", "dvar"): (1.63e-07, 4.060e-08),
    ("det", "R1-K4-alea4-extremes", "dbox"): (4.79e-04, 1.197e-04),
    ("det", "R1-K4-alea4-extremes", "dvar"): (1.05e-04, 2.607e-05),
    ("det", "R255-K4-alea4-extremes", "dbox"): (4.05e-06, 1.011e-06),
    ("det", "R255-K4-alea4-extremes", "dvar"): (2.36e-05, 5.876e-06),
    ("det", "R257-K4-alea4-extremes", "dbox"): (2.76e-06, 6.898e-07),
    ("det", "R257-K4-alea4-extremes", "dvar"): (2.99e-05, 7.456e-06),
    ("det", "R4096-K4-alea4-extremes", "dbox"): (3.47e-07, 8.671e-08),
    ("det", "R4096-K4-alea4-extremes", "dvar"): (2.18e-06, 5.446e-07),
    ("det", "R257-K2-alea4-extremes", "dbox"): (1.96e-06, 4.892e-07),
    ("det", "R257-K2-alea4-extremes", "dvar"): (1.81e-05, 4.519e-06),
    ("det", "R257-K9-alea4-extremes", "dbox"): (2.23e-06, 5.570e-07),
    ("det", "R257-K9-alea4-extremes", "dvar"): (2.26e-05, 5.631e-06),
    ("det", "R1-K4-alea7-normal", "dcls"): (1.04e-07, 2.578e-08),
    ("det", "R1-K4-alea7-normal", "dvar"): (1.50e-06, 3.731e-07),
    ("det", "R1-K4-alea7-wide", "dbox"): (4.23e-07, 1.057e-07),
    ("det", "R1-K4-alea7-wide", "dvar"): (8.96e-07, 2.239e-07),
    ("det", "R1-K4-alea7-no_fg", "dcls"): (1.24e-07, 3.100e-08),
    ("det", "R1-K4-alea7-breakpoints", "dcls"): (2.07e-07, 5.167e-08),
    ("det", "R1-K4-alea7-breakpoints", "dvar"): (2.25e-07, 5.606e-08),
    ("det", "R1-K4-alea7-extremes", "dbox"): (6.57e-04, 1.641e-04),
    ("det", "R1-K4-alea7-extremes", "dvar"): (5.60e-04, 1.398e-04),
    ("det", "R255-K4-alea7-extremes", "dbox"): (1.82e-05, 4.543e-06),
    ("det", "R255-K4-alea7-extremes", "dvar"): (6.16e-05, 1.538e-05),
    ("det", "R257-K4-alea7-extremes", "dbox"): (7.31e-06, 1.826e-06),
    ("det", "R257-K4-alea7-extremes", "dvar"): (5.53e-05, 1.381e-05),
    ("det", "R4096-K4-alea7-extremes", "dbox"): (9.65e-07, 2.412e-07),
    ("det", "R4096-K4-alea7-extremes", "dvar"): (5.28e-06, 1.319e-06),
    ("det", "R257-K2-alea7-extremes", "dbox"): (1.07e-05, 2.653e-06),
    ("det", "R257-K2-alea7-extremes", "dvar"): (6.26e-05, 1.563e-05),
    ("det", "R257-K9-alea7-extremes", "dbox"): (5.67e-06, 1.415e-06),
    ("det", "R257-K9-alea7-extremes", "dvar"): (4.96e-05, 1.238e-05),
}


def _ops():
    from faster_rcnn_pytorch_multimodal_amd import ops
    return ops


def _hip_error():
    from faster_rcnn_pytorch_multimodal_amd import _hip
    return _hip.HipError


def _dev(inp, *names):
    return [inp[n].to(DEV) for n in names]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _scale(t):
    return max(1.0, float(t.detach().abs().max())) if t.numel() else 1.0


def _check(section, case, name, got, ref, bar, side, headroom=1.0):
    """max |got - ref| / bar <= 1 / headroom; bar is a number or a tensor shaped like ref.  Prints the figure first."""
    bar = WIDENED.get((section, case, name), (bar,))[0]
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    ref = torch.as_tensor(ref).detach().double().reshape(-1)
    assert got.shape == ref.shape, (section, case, name, got.shape, ref.shape)
    assert bool(torch.isfinite(ref).all()), (section, case, name, "reference not finite")
    assert bool(torch.isfinite(got).all()), (section, case, name, "result not finite")
    bar_t = torch.as_tensor(bar, dtype=torch.float64).reshape(-1)
    err = (got - ref).abs()
    ratio = float((err / bar_t).max())
    print("LSK|%s|%s|%s|%s|err=%.3e|ratio=%.4f" % (section, side, case, name, float(err.max()), ratio))
    assert ratio * headroom <= 1.0, "%s %s %s (%s): max err %.3e is %.3f of its bar, allowed %.3f" % (
        section, case, name, side, float(err.max()), ratio, 1.0 / headroom)


def _check_all(section, case, got, ref, bars, side, headroom=1.0):
    for name in ref:
        _check(section, case, name, got[name], ref[name], bars[name], side, headroom)


def _huber32(diff):
    a = diff.abs()
    return torch.where(a < 1, 0.5 * (diff * diff), a - 0.5), torch.where(a < 1, diff, torch.sign(diff))


BREAK_DIFFS = torch.tensor([-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5])


def _breakpoint_pairs(shape, g):
    """Dyadic (pred, target) with pred - target cycling through BREAK_DIFFS exactly in fp32 and fp64."""
    n = int(np.prod(shape))
    tgt = torch.randint(-8, 9, (n,), generator=g).float() / 4
    pred = tgt + BREAK_DIFFS[torch.arange(n) % 7]
    want = BREAK_DIFFS[torch.arange(n) % 7]
    assert torch.equal(pred - tgt, want) and torch.equal(pred.double() - tgt.double(), want.double())
    return pred.view(shape), tgt.view(shape)


# ================================================================================================
# 1. rpn_loss
# ================================================================================================
RPN_SHAPES = [(3, 5, 30), (204, 25, 152), (211, 9, 56), (4400, 15, 96)]
RPN_VARIANTS = ["normal", "wide", "none_labelled", "all_fg", "breakpoints"]
RPN_CASES = [(s, v) for s in RPN_SHAPES for v in RPN_VARIANTS]
RPN_G = (0.7, 1.3)


def _rpn_id(c):
    return "hw%d-A%d-ld%d-%s" % (c[0] + (c[1],))


@functools.lru_cache(maxsize=None)
def rpn_case(shape, variant):
    hw, a, ld = shape
    total = hw * a
    g = torch.Generator().manual_seed(77 + hw + 1000 * RPN_VARIANTS.index(variant))
    rpn = torch.randn(hw, ld, generator=g)
    labels = torch.randint(-1, 2, (total,), generator=g).float()
    targets = torch.randn(total, 4, generator=g) * 1.5
    box_labels = labels                       # the anchors that carry box weights (anchor_target_layer's labels)
    if variant == "wide":
        sign = torch.randint(0, 2, (hw, 1), generator=g).float() * 2 - 1
        rpn[:, :2 * a] = rpn[:, :2 * a] * 30 + 50 * sign
    elif variant == "none_labelled":
        labels = torch.full((total,), -1.0)   # box weights stay: the box loss is independent of the labels
    elif variant == "all_fg":
        labels = box_labels = torch.ones(total)
    inside = (box_labels == 1).float().view(-1, 1).expand(-1, 4).contiguous()
    outside = ((box_labels >= 0).float() / max(1.0, float((box_labels >= 0).sum()))).view(-1, 1).expand(-1, 4).contiguous()
    if variant == "breakpoints":
        inside = (torch.arange(total) % 4 == 0).float().view(-1, 1).expand(-1, 4).contiguous()
        outside = inside / 64
        pred, targets = _breakpoint_pairs((total, 4), g)
        rpn[:, 2 * a:6 * a] = pred.view(hw, 4 * a)
    inp = dict(rpn=rpn.contiguous(), labels=labels, targets=targets.contiguous(), inside=inside, outside=outside, a=a)
    # float64 reference: autograd of grad_ce * ce + grad_box * box
    rd = rpn.double().requires_grad_(True)
    logits = torch.stack((rd[:, :a].reshape(-1), rd[:, a:2 * a].reshape(-1)), 1)          # (HWA, 2): [bg, fg]
    sel = labels >= 0
    count = int(sel.sum())
    if count:
        ce = F.cross_entropy(logits[sel], labels[sel].long())
        ce_terms = F.cross_entropy(logits[sel], labels[sel].long(), reduction="none").detach()
    else:                                     # the device defines the mean over no anchor as 0 (cnt > 0 ? ce / cnt : 0)
        ce, ce_terms = rd.sum() * 0, torch.zeros(1, dtype=torch.float64)
    v = lambda t: t.double().view(1, hw, 1, 4 * a)
    box = O.smooth_l1_loss("RPN", rd[:, 2 * a:6 * a].reshape(1, hw, 1, 4 * a), v(targets), v(inside), v(outside), dim=(1, 2, 3))
    (RPN_G[0] * ce + RPN_G[1] * box).backward()
    box_terms = outside.double() * O.huber_loss(rpn[:, 2 * a:6 * a].double().reshape(total, 4) * inside.double(),
                                                targets.double() * inside.double())
    ref = dict(ce=ce.detach(), box=box.detach(), drpn=rd.grad)
    bars = dict(ce=1e-5 * _scale(ce_terms), box=1e-5 * _scale(box_terms), drpn=1e-6 * _scale(rd.grad))
    return inp, ref, bars, count


def _serial_sum32(v):
    s = np.float32(0)
    for x in v.numpy():
        s = np.float32(s + x)
    return s


def _rpn_block_sum32(v, total):
    """256 block partials of ceil(total / 256) anchors each, then the partials in block order, all in fp32."""
    per = (total + 255) // 256
    return _serial_sum32(F.pad(v, (0, 256 * per - total)).view(256, per).sum(1))


def rpn_restate(inp):
    rpn, labels, t, iw, ow, a = (inp[k] for k in ("rpn", "labels", "targets", "inside", "outside", "a"))
    hw, ld = rpn.shape
    total = hw * a
    bg, fg = rpn[:, :a].reshape(-1), rpn[:, a:2 * a].reshape(-1)
    on, is_fg = labels >= 0, labels > 0.5
    m = torch.maximum(bg, fg)
    eb, ef = torch.exp(bg - m), torch.exp(fg - m)
    lse = m + torch.log(eb.double() + ef.double()).float()
    zero = torch.zeros(())
    ce_sum = _rpn_block_sum32(torch.where(on, lse - torch.where(is_fg, fg, bg), zero), total)
    cnt = np.float32(int(on.sum()))
    p = rpn[:, 2 * a:6 * a].reshape(total, 4)
    h, hg = _huber32(p * iw - t * iw)
    box = _rpn_block_sum32((ow * h).sum(1), total)
    inv = np.float32(RPN_G[0]) / cnt if cnt > 0 else np.float32(0)
    drpn = torch.zeros(hw, ld)
    drpn[:, :a] = torch.where(on, (eb / (eb + ef) - (~is_fg).float()) * float(inv), zero).view(hw, a)
    drpn[:, a:2 * a] = torch.where(on, (ef / (eb + ef) - is_fg.float()) * float(inv), zero).view(hw, a)
    drpn[:, 2 * a:6 * a] = (((torch.tensor(RPN_G[1]) * ow) * hg) * iw).view(hw, 4 * a)
    ce = ce_sum / cnt if cnt > 0 else np.float32(0)
    return dict(ce=torch.tensor(float(ce)), box=torch.tensor(float(box)), drpn=drpn), int(cnt)


@pytest.mark.parametrize("case", RPN_CASES, ids=_rpn_id)
def test_cpu_restatement_rpn_loss(case):
    inp, ref, bars, count = rpn_case(*case)
    got, cnt = rpn_restate(inp)
    assert cnt == count
    _check_all("rpn", _rpn_id(case), got, ref, bars, "cpu32", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RPN_CASES, ids=_rpn_id)
def test_rpn_loss(hip, case):
    ops = _ops()
    inp, ref, bars, count = rpn_case(*case)
    a = inp["a"]
    args = _dev(inp, "rpn") + [a] + _dev(inp, "labels", "targets", "inside", "outside")
    losses, drpn = ops.rpn_loss(*args, RPN_G[0], RPN_G[1])
    lo = losses.cpu()
    assert float(lo[2]) == float(count)                                          # labelled count: exact
    _check_all("rpn", _rpn_id(case), dict(ce=lo[0], box=lo[1], drpn=drpn), ref, bars, "device")
    assert bool((drpn[:, 6 * a:] == 0).all())                                    # padding columns
    if case[1] == "none_labelled":
        assert float(lo[0]) == 0.0 and float(lo[2]) == 0.0 and bool((drpn[:, :2 * a] == 0).all())
    losses2, drpn2 = ops.rpn_loss(*args, RPN_G[0], RPN_G[1])
    assert _bits_equal(losses, losses2) and _bits_equal(drpn, drpn2)             # deterministic
    losses3, none = ops.rpn_loss(*args, RPN_G[0], RPN_G[1], want_grad=False)
    assert none is None and _bits_equal(losses, losses3)


# ================================================================================================
# 2. det_loss: plain, LiDAR, aleatoric
# ================================================================================================
LIDAR_W = (1.0, 2.0, 0.5, 1.0, 1.5, 3.0, 0.25)
# form -> (E, net_type of the oracle, per-element weights / sin on element 6, aleatoric)
DET_FORMS = {"plain4": (4, "image", None, False), "lidar7": (7, "lidar", LIDAR_W, False),
             "alea4": (4, "image", None, True), "alea7": (7, "lidar", LIDAR_W, True)}
DET_SHAPES = [(1, 4), (255, 4), (257, 4), (4096, 4), (257, 2), (257, 9)]
DET_VARIANTS = ["normal", "wide", "no_fg", "breakpoints"]
DET_CASES = [(r, k, f, v) for f in DET_FORMS for (r, k) in DET_SHAPES
             for v in DET_VARIANTS + (["extremes"] if DET_FORMS[f][3] else [])]
DET_G = (0.6, 1.7)


def _det_id(c):
    return "R%d-K%d-%s-%s" % c


@contextlib.contextmanager
def _oracle_lidar_weights(w):
    old = O.LIDAR_REG_LOSS_WEIGHT
    O.LIDAR_REG_LOSS_WEIGHT = tuple(w) if w is not None else old
    try:
        yield
    finally:
        O.LIDAR_REG_LOSS_WEIGHT = old


@functools.lru_cache(maxsize=None)
def det_case(r, k, form, variant):
    e, net_type, w, alea = DET_FORMS[form]
    cols = e * k
    g = torch.Generator().manual_seed(r * 31 + k * 7 + 100 * DET_VARIANTS.index(variant) if variant != "extremes" else r + k)
    cls = torch.randn(r, k, generator=g) * (40.0 if variant == "wide" else 1.0)
    lab = torch.randint(0, k, (r,), generator=g).float()
    lab[0] = k - 1                                                  # at least one foreground row, also for R = 1
    if variant == "no_fg":
        lab = torch.zeros(r)
    bp, bt = torch.randn(r, cols, generator=g), torch.randn(r, cols, generator=g) * 2
    if variant == "breakpoints":
        bp, bt = _breakpoint_pairs((r, cols), g)                    # sin(+-1.5) = +-0.997: no sine of +-1 on the yaw
    iw = torch.zeros(r, cols)                                       # as proposal_target_layer: the labelled class's E
    for c in range(1, k):                                           # columns of foreground rows
        iw[lab == c, e * c:e * c + e] = 1.0
    ow = (iw > 0).float()
    bv = None
    if alea:
        bv = torch.randn(r, cols, generator=g) * 0.5
        if variant == "extremes":
            bv = torch.tensor([-8.0, 0.0, 8.0])[torch.arange(r * cols) % 3].view(r, cols).contiguous()
    inp = dict(cls=cls, lab=lab, bp=bp.contiguous(), bt=bt.contiguous(), iw=iw, ow=ow, bv=bv, form=form)
    csd, bpd = cls.double().requires_grad_(True), bp.double().requires_grad_(True)
    bvd = bv.double().requires_grad_(True) if alea else None
    ce = F.cross_entropy(csd, lab.long())
    with _oracle_lidar_weights(w):
        bl = O.smooth_l1_loss("DET", bpd, bt.double(), iw.double(), ow.double(), net_type=net_type, bbox_var=bvd)
    (DET_G[0] * ce + DET_G[1] * bl).backward()
    # per-element terms of the reference (for the bars only): loss_utils.py:61-85 element by element
    with torch.no_grad():
        p, t = (bp.double() * iw.double()).view(-1, e), (bt.double() * iw.double()).view(-1, e)
        el = O.huber_loss(p, t)
        if w is not None:
            el[:, 6] = O.huber_loss(p[:, 6], t[:, 6], sin_en=True)
            el = el * torch.tensor(w, dtype=torch.float64)
        el = el.view(r, cols)
        if alea:
            el = (0.5 * el * torch.exp(-bv.double()) + 0.5 * bv.double()) * iw.double()
        el = ow.double() * el
        assert abs(float(el.sum(1).mean()) - float(bl)) <= 1e-12 * _scale(el) * cols
        ce_terms = F.cross_entropy(cls.double(), lab.long(), reduction="none")
    ref = dict(ce=ce.detach(), box=bl.detach(), dcls=csd.grad, dbox=bpd.grad)
    bars = dict(ce=1e-5 * _scale(ce_terms), box=1e-5 * _scale(el), dcls=1e-7 * _scale(csd.grad), dbox=1e-7 * _scale(bpd.grad))
    if alea:
        ref["dvar"], bars["dvar"] = bvd.grad, 1e-7 * _scale(bvd.grad)
    return inp, ref, bars


def _thread_sum32(v):
    """Thread t of the one workgroup sums rows t, t + 256, ...; then the 256 thread sums."""
    return F.pad(v, (0, -v.numel() % 256)).view(-1, 256).sum(0).sum()


def det_restate(inp):
    cls, lab, bp, bt, iw, ow, bv = (inp[n] for n in ("cls", "lab", "bp", "bt", "iw", "ow", "bv"))
    e, _, w, alea = DET_FORMS[inp["form"]]
    r, k = cls.shape
    rf = torch.tensor(float(r))
    m = cls.max(1, keepdim=True).values
    ex = torch.exp(cls - m)
    s = ex.double().sum(1, keepdim=True)
    onehot = F.one_hot(lab.long(), k).float()
    ce_rows = (m + torch.log(s).float()).view(-1) - (cls * onehot).sum(1)
    dcls = ((ex.double() / s).float() - onehot) * (torch.tensor(DET_G[0]) / rf)
    diff, chain = bp * iw - bt * iw, iw.clone()
    we = torch.ones(e)
    if w is not None:
        we = torch.tensor(w)
        sin_col = (torch.arange(bp.shape[1]) % e == 6).expand_as(bp)
        chain = torch.where(sin_col, chain * torch.cos(diff), chain)
        diff = torch.where(sin_col, torch.sin(diff), diff)
    we = we.repeat(k)
    h, hg = _huber32(diff)
    l, gb = h * we, torch.tensor(DET_G[1]) / rf
    out = {}
    if alea:
        ev = torch.exp(-bv)
        el = ow * ((0.5 * l * ev + 0.5 * bv) * iw)
        out["dbox"] = gb * ow * iw * (0.5 * ev) * (hg * we) * chain
        out["dvar"] = gb * ow * iw * (0.5 - 0.5 * l * ev)
    else:
        el = ow * l
        out["dbox"] = gb * ow * (hg * we) * chain
    out.update(ce=_thread_sum32(ce_rows) / rf, box=_thread_sum32(el.sum(1)) / rf, dcls=dcls)
    return out


@pytest.mark.parametrize("case", DET_CASES, ids=_det_id)
def test_cpu_restatement_det_loss(case):
    inp, ref, bars = det_case(*case)
    _check_all("det", _det_id(case), det_restate(inp), ref, bars, "cpu32", HEADROOM)


def _run_det(ops, inp, want_grad=True):
    e, _, w, alea = DET_FORMS[inp["form"]]
    cls, lab, bp, bt, iw, ow = _dev(inp, "cls", "lab", "bp", "bt", "iw", "ow")
    if alea:
        losses, dcls, dbox, dvar = ops.det_loss_aleatoric(cls, lab, bp, inp["bv"].to(DEV), bt, iw, ow, bbox_elem=e, weights=w,
                                                          ry_sin=w is not None, grad_ce=DET_G[0], grad_box=DET_G[1])
        return dict(losses=losses, dcls=dcls, dbox=dbox, dvar=dvar)
    losses, dcls, dbox = ops.det_loss(cls, lab, bp, bt, iw, ow, bbox_elem=e, grad_ce=DET_G[0], grad_box=DET_G[1],
                                      want_grad=want_grad, lidar=(w, True) if w is not None else None)
    return dict(losses=losses, dcls=dcls, dbox=dbox)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DET_CASES, ids=_det_id)
def test_det_loss(hip, case):
    ops = _ops()
    inp, ref, bars = det_case(*case)
    got = _run_det(ops, inp)
    lo = got["losses"].cpu()
    _check_all("det", _det_id(case), dict(got, ce=lo[0], box=lo[1]), ref, bars, "device")
    if case[3] == "no_fg":
        assert float(lo[1]) == 0.0 and bool((got["dbox"] == 0).all())
        assert "dvar" not in got or bool((got["dvar"] == 0).all())
    again = _run_det(ops, inp)
    assert all(_bits_equal(got[n], again[n]) for n in got)                       # deterministic
    if not DET_FORMS[case[2]][3]:
        no_grad = _run_det(ops, inp, want_grad=False)
        assert no_grad["dcls"] is None and no_grad["dbox"] is None and _bits_equal(no_grad["losses"], got["losses"])


@pytest.mark.gpu
def test_det_loss_rejects_bad_shapes(hip):
    """FRCNN_REQUIRE / the wrapper refuse these on the host: nothing is launched."""
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(_hip_error()):
        ops.det_loss(z(4097, 2), z(4097), z(4097, 8), z(4097, 8), z(4097, 8), z(4097, 8))
    with pytest.raises(_hip_error()):
        ops.det_loss_aleatoric(z(4097, 2), z(4097), z(4097, 8), z(4097, 8), z(4097, 8), z(4097, 8), z(4097, 8))
    with pytest.raises(_hip_error()):
        ops.det_loss(z(8, 2), z(8), z(8, 8), z(8, 8), z(8, 8), z(8, 8), lidar=([1.0] * 7, True))      # 4*K wide, not 7*K


# ================================================================================================
# 3. bayesian_cross_entropy, logit_distort, dropout
# ================================================================================================
BAYES_SHAPES = [(1, 2, 3), (257, 3, 50), (300, 16, 20)]
BAYES_CASES = [(s, m) for s in BAYES_SHAPES for m in ("logvar", "var")]
BAYES_SEED, BAYES_STREAM, BAYES_GRAD = 11, O.UC_STREAM["bayes_ce"], 0.8


def _bayes_id(c):
    return "N%d-K%d-S%d-%s" % (c[0] + (c[1],))


@functools.lru_cache(maxsize=None)
def bayes_case(shape, mode):
    n, k, s = shape
    g = torch.Generator().manual_seed(n + k + s)
    score = torch.randn(n, k, generator=g).clamp(-4, 4)
    logvar = (torch.randn(n, k, generator=g) * 0.7 - 0.5).clamp(max=1.0)
    labels = torch.randint(0, k, (n,), generator=g).float()
    sc = score.double().requires_grad_(True)
    if mode == "logvar":
        var_in, planted = logvar, 0
        leaf = logvar.double().requires_grad_(True)
        var64 = torch.exp(leaf)
    else:
        var_in = torch.exp(logvar)
        var_in.view(-1)[::5] = 0.0                                  # variance exactly 0: the sd == 0 branch
        planted = int((var_in == 0).sum())
        assert planted == (n * k + 4) // 5
        leaf = var_in.double().requires_grad_(True)
        var64 = leaf
    loss, _ = O.bayesian_cross_entropy(sc, var64, labels, s, BAYES_SEED, BAYES_STREAM)
    (BAYES_GRAD * loss).backward()
    with torch.no_grad():                                           # the reference's per-RoI mean probability
        samples, _ = O.logit_distort_replay(score.double(), var64.detach(), s, BAYES_SEED, BAYES_STREAM)
        avg = F.softmax(samples, 2).mean(0).gather(1, labels.long().unsqueeze(1))
    assert float(score.abs().max()) <= 4 and float(logvar.max()) <= 1 and float(avg.min()) > 1e-6
    dvar = leaf.grad.clone()
    zero_var = var_in == 0 if mode == "var" else torch.zeros_like(var_in, dtype=torch.bool)
    # autograd of sqrt at 0 is inf / nan (0 * inf); the device defines dvar = 0 there.  Nothing else is left out.
    assert int(zero_var.sum()) == planted and bool(torch.isfinite(dvar[~zero_var]).all())
    dvar[zero_var] = 0.0
    inp = dict(score=score, var=var_in.contiguous(), labels=labels, s=s, is_log=mode == "logvar", zero_var=zero_var)
    ref = dict(loss=loss.detach(), dscore=sc.grad, dvar=dvar)
    bars = dict(loss=2e-5 * _scale(-torch.log(avg)), dscore=2e-6 * _scale(sc.grad),
                dvar=(2e-6 if mode == "logvar" else 5e-6) * _scale(dvar))
    return inp, ref, bars


def bayes_restate(inp):
    score, var, labels, s, is_log = (inp[n] for n in ("score", "var", "labels", "s", "is_log"))
    n, k = score.shape
    eps = torch.from_numpy(O.normal01(BAYES_SEED, BAYES_STREAM, np.arange(n * k * s))).view(s, n, k)
    sd = torch.sqrt(torch.exp(var) if is_log else var)
    z = score[None] + sd[None] * eps
    ez = torch.exp(z - z.max(2, keepdim=True).values)
    p = ez / ez.sum(2, keepdim=True)
    onehot = F.one_hot(labels.long(), k).float()[None]
    pt = (p * onehot).sum(2, keepdim=True)
    avg = pt.sum(0) / s
    d = pt * (onehot - p)
    gs, gv = d.sum(0), (d * eps).sum(0)
    c = -BAYES_GRAD / (float(n) * float(s) * avg)
    dvar = c * gv * sd * 0.5 if is_log else torch.where(sd > 0, c * gv / (2.0 * sd), torch.zeros(()))
    return dict(loss=(-torch.log(avg)).mean(), dscore=c * gs, dvar=dvar)


@pytest.mark.parametrize("case", BAYES_CASES, ids=_bayes_id)
def test_cpu_restatement_bayesian_cross_entropy(case):
    inp, ref, bars = bayes_case(*case)
    _check_all("bayes", _bayes_id(case), bayes_restate(inp), ref, bars, "cpu32", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("case", BAYES_CASES, ids=_bayes_id)
def test_bayesian_cross_entropy(hip, case):
    ops = _ops()
    inp, ref, bars = bayes_case(*case)
    args = _dev(inp, "score", "var", "labels") + [inp["s"], BAYES_SEED, BAYES_STREAM]
    loss, dscore, dvar = ops.bayesian_cross_entropy(*args, grad=BAYES_GRAD, var_is_log=inp["is_log"])
    assert bool((dvar.cpu()[inp["zero_var"]] == 0).all())                        # sd == 0: the device defines 0
    _check_all("bayes", _bayes_id(case), dict(loss=loss, dscore=dscore, dvar=dvar), ref, bars, "device")
    loss2, none1, none2 = ops.bayesian_cross_entropy(*args, grad=BAYES_GRAD, var_is_log=inp["is_log"], want_grad=False)
    assert none1 is None and none2 is None and _bits_equal(loss, loss2)


@pytest.mark.gpu
def test_bayesian_cross_entropy_rejects_17_classes(hip):
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(_hip_error()):
        ops.bayesian_cross_entropy(z(4, 17), z(4, 17), z(4), 3, 1, 16)


DISTORT_CASES = [(37, 3, 1, True), (37, 3, 5, False), (1, 2, 1, False)]          # n*S = 111, 555, 2: never 256-aligned
DISTORT_SEED, DISTORT_STREAM = 5, O.UC_STREAM["logit_distort"]


def _distort_id(c):
    return "N%d-K%d-S%d-%s" % (c[0], c[1], c[2], "logvar" if c[3] else "var")


@functools.lru_cache(maxsize=None)
def distort_case(n, k, s, is_log):
    g = torch.Generator().manual_seed(n * k + s)
    score, logvar = torch.randn(n, k, generator=g), torch.randn(n, k, generator=g) * 0.5
    var_in = logvar if is_log else torch.exp(logvar)
    var64 = torch.exp(logvar.double()) if is_log else var_in.double()
    samples, _ = O.logit_distort_replay(score.double(), var64, s, DISTORT_SEED, DISTORT_STREAM)
    # 2e-5: the existing bar (logf / cosf of the Box-Muller draw differ from numpy's in the last ulps); variance 2e-6 rel
    return dict(score=score, var=var_in.contiguous(), s=s, is_log=is_log), dict(samples=samples, var=var64), \
        dict(samples=2e-5 * _scale(samples), var=2e-6 * var64)


def distort_restate(inp):
    score, var, s = inp["score"], inp["var"], inp["s"]
    eps = torch.from_numpy(O.normal01(DISTORT_SEED, DISTORT_STREAM, np.arange(score.numel() * s))).view((s,) + score.shape)
    v = torch.exp(var) if inp["is_log"] else var
    return dict(samples=score[None] + torch.sqrt(v)[None] * eps, var=v)


@pytest.mark.parametrize("case", DISTORT_CASES, ids=_distort_id)
def test_cpu_restatement_logit_distort(case):
    inp, ref, bars = distort_case(*case)
    _check_all("distort", _distort_id(case), distort_restate(inp), ref, bars, "cpu32", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DISTORT_CASES, ids=_distort_id)
def test_logit_distort(hip, case):
    ops = _ops()
    inp, ref, bars = distort_case(*case)
    samples, var = ops.logit_distort(inp["score"].to(DEV), inp["var"].to(DEV), inp["s"], DISTORT_SEED, DISTORT_STREAM,
                                     var_is_log=inp["is_log"])
    assert samples.shape == (inp["s"],) + inp["score"].shape
    _check_all("distort", _distort_id(case), dict(samples=samples, var=var), ref, bars, "device")


@functools.lru_cache(maxsize=None)
def dropout_p0_case(repeat):
    g = torch.Generator().manual_seed(repeat)
    x = torch.randn(37, 13, generator=g)
    dy = torch.randn((repeat, 37, 13) if repeat > 1 else (37, 13), generator=g)
    ref = dy.double().reshape(repeat, 37, 13).sum(0)
    # `repeat` roundings of partial sums <= repeat * max|dy|, 4x headroom
    return dict(x=x, dy=dy, repeat=repeat), dict(dx=ref), dict(dx=4 * repeat * repeat * U / 2 * _scale(dy))


def dropout_p0_restate(inp):
    dy = inp["dy"].reshape(inp["repeat"], 37, 13)
    dx = torch.zeros(37, 13)
    for t in range(inp["repeat"]):
        dx = dx + dy[t] * 1.0
    return dict(dx=dx)


@pytest.mark.parametrize("repeat", [1, 6])
def test_cpu_restatement_dropout_p0(repeat):
    inp, ref, bars = dropout_p0_case(repeat)
    _check_all("dropout", "p0-repeat%d" % repeat, dropout_p0_restate(inp), ref, bars, "cpu32", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("repeat", [1, 6])
def test_dropout_p0_is_identity_and_backward_sums_copies(hip, repeat):
    ops = _ops()
    inp, ref, bars = dropout_p0_case(repeat)
    y = ops.dropout(inp["x"].to(DEV), 0.0, 3, 11, repeat=repeat).cpu()
    want = inp["x"] if repeat == 1 else inp["x"].unsqueeze(0).expand(repeat, -1, -1)
    assert _bits_equal(y, want.contiguous())
    dx = ops.dropout_bwd(inp["dy"].to(DEV), 0.0, 3, 11, repeat=repeat)
    _check_all("dropout", "p0-repeat%d" % repeat, dict(dx=dx), ref, bars, "device")


@pytest.mark.gpu
def test_dropout_grid_stride_second_trip(hip):
    """300 * 1024 * 7 = 2150400 > 8192 * 256 outputs: the masks past the first trip still replay bit for bit."""
    ops = _ops()
    x = torch.randn(300, 1024, generator=torch.Generator().manual_seed(9))
    assert x.numel() * 7 > GRID_CAP
    y = ops.dropout(x.to(DEV), 0.3, 99, 13, repeat=7).cpu()
    assert torch.equal(y, O.dropout_replay(x, 0.3, 99, 13, repeat=7))


# ================================================================================================
# 4. mc_bbox_var, mc_cls_stats, mc_mean, exp
# ================================================================================================
# (sum x^2 - (sum x)^2 / T) / (T - 1) is the reference's formula (loss_utils.py:114-120) and cancels by design: its fp32
# error is proportional to T max(x^2) / (T - 1), not to the variance.  Worst case over the T squares, 2(T - 1) additions,
# the product and the two divisions is about (2T + 2) * 2^-23 * T max(x^2) / (T - 1); roundings average out, and the
# sequential fp32 restatement (the kernel's own order, contraction off) reaches 3.71 of 2^-23 T max(x^2) / (T - 1) on
# these cases (T = 10, mean 50, n = 8192*256+77) and 4.0000002 on the softmax variance of ten equal samples.  C_VAR is
# the next integer above 4x the measured 4.0000002, and stays below the worst case for T = 10.
C_VAR = 17.0


def _var_bar(t, x):
    return C_VAR * U * t * float((x.double() ** 2).max()) / (t - 1)


def _var_seq32(x):
    t = x.shape[0]
    s, q = torch.zeros_like(x[0]), torch.zeros_like(x[0])
    for i in range(t):
        s, q = s + x[i], q + x[i] * x[i]
    r = (q + -(s * s) / float(t)) / float(t - 1)
    return torch.where(r > 0, r, torch.zeros(()))


def _two_pass_var64(x):
    x = x.double()
    return ((x - x.mean(0)) ** 2).sum(0) / (x.shape[0] - 1)


BBOX_VAR_CASES = [(t, n, ms) for t in (2, 10) for n in (1, 300 * 8) for ms in ((0.0, 1.0), (3.0, 0.5), (50.0, 0.5))] + \
                 [(2, BIG, (3.0, 0.5)), (10, BIG, (50.0, 0.5)), (10, 300 * 8, "constant"), (2, 300 * 8, "constant")]


def _bbox_var_id(c):
    return "T%d-n%d-%s" % (c[0], c[1], c[2] if isinstance(c[2], str) else "m%g-s%g" % c[2])


def bbox_var_case(t, n, ms):            # not cached: the large stacks are built once per test and dropped
    g = torch.Generator().manual_seed(t * 13 + n % 1000)
    if ms == "constant":
        x = (torch.randn(1, n, generator=g) * 20 + 50.3).expand(t, n).contiguous()
    else:
        x = ms[0] + ms[1] * torch.randn(t, n, generator=g)
    ref = _two_pass_var64(x)
    # the oracle's own formula in float64 agrees with the two-pass variance far inside the bar
    assert float((O.compute_bbox_var(x.double()) - ref).abs().max()) <= 1e-3 * _var_bar(t, x)
    return dict(x=x), dict(var=ref), dict(var=_var_bar(t, x))


@pytest.mark.parametrize("case", BBOX_VAR_CASES, ids=_bbox_var_id)
def test_cpu_restatement_mc_bbox_var(case):
    inp, ref, bars = bbox_var_case(*case)
    got = _var_seq32(inp["x"])
    assert bool((got >= 0).all())
    _check_all("bbox_var", _bbox_var_id(case), dict(var=got), ref, bars, "cpu32", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("case", BBOX_VAR_CASES, ids=_bbox_var_id)
def test_mc_bbox_var(hip, case):
    ops = _ops()
    inp, ref, bars = bbox_var_case(*case)
    var = ops.mc_bbox_var(inp["x"].to(DEV))
    assert var.shape == (case[1],) and bool((var >= 0).all())                    # clamped: never negative
    _check_all("bbox_var", _bbox_var_id(case), dict(var=var), ref, bars, "device")


@pytest.mark.gpu
def test_mc_bbox_var_rejects_one_sample(hip):
    with pytest.raises(_hip_error()):
        _ops().mc_bbox_var(torch.zeros(1, 8, device=DEV))


CLS_STATS_CASES = [(t, n, k, "random") for t in (1, 2, 10) for n in (1, 300 * 8) for k in (2, 5)] + \
                  [(2, BIG, 2, "random"), (10, 300 * 8, 5, "equal"), (2, 300 * 8, 2, "equal")]


def _cls_stats_id(c):
    return "T%d-N%d-K%d-%s" % c


def cls_stats_case(t, n, k, kind):
    g = torch.Generator().manual_seed(t * 7 + k + n % 1000)
    if kind == "equal":
        scores = (torch.randn(1, n, k, generator=g) * 5).clamp(-15, 15).expand(t, n, k).contiguous()
    else:
        scores = (torch.randn(t, n, k, generator=g) * 5).clamp(-15, 15)         # spread <= 30: exp(-30) = 9e-14 > FLT_MIN
    assert float(scores.max() - scores.min()) <= 30
    s64 = scores.double()
    prob = F.softmax(s64, 2)
    mean_prob = prob.mean(0)
    ent = O.categorical_entropy(mean_prob)
    mi = O.categorical_mutual_information(s64)
    # T = 1: the reference's formula divides by T - 1 = 0; the device defines the variance of one sample as 0
    var = _two_pass_var64(prob) if t > 1 else torch.zeros(n, k, dtype=torch.float64)
    ref = dict(mean_prob=mean_prob, entropy=ent, mutual_info=mi, prob_var=var)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    if kind == "equal":
        assert float(mi.abs().max()) <= 1e-12 and float(var.abs().max()) <= 1e-20
    # the existing bars (tests/test_gpu_parity.py): rtol / atol per element; the variance as mc_bbox_var with x = p <= 1
    bars = dict(mean_prob=2e-6 * mean_prob + 1e-7, entropy=2e-6 * ent.abs() + 2e-6, mutual_info=1e-5 * mi.abs() + 3e-6,
                prob_var=C_VAR * U * t / max(t - 1, 1))
    return dict(scores=scores), ref, bars


def cls_stats_restate(inp):
    s = inp["scores"]
    t = s.shape[0]
    ez = torch.exp(s - s.max(2, keepdim=True).values)
    p = ez / ez.sum(2, keepdim=True)
    plogp = (p * torch.log2(p)).sum(2).sum(0)
    mean = p.sum(0) / float(t)
    h = (mean * torch.log2(mean)).sum(1)
    var = _var_seq32(p) if t > 1 else torch.zeros_like(mean)
    return dict(mean_prob=mean, entropy=-h, mutual_info=plogp / float(t) + -h, prob_var=var)


@pytest.mark.parametrize("case", CLS_STATS_CASES, ids=_cls_stats_id)
def test_cpu_restatement_mc_cls_stats(case):
    inp, ref, bars = cls_stats_case(*case)
    _check_all("cls_stats", _cls_stats_id(case), cls_stats_restate(inp), ref, bars, "cpu32", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CLS_STATS_CASES, ids=_cls_stats_id)
def test_mc_cls_stats(hip, case):
    ops = _ops()
    inp, ref, bars = cls_stats_case(*case)
    x = inp["scores"].to(DEV)
    mean_prob, ent, mi, var = ops.mc_cls_stats(x, want_var=True)
    got = dict(mean_prob=mean_prob, entropy=ent, mutual_info=mi, prob_var=var)
    _check_all("cls_stats", _cls_stats_id(case), got, ref, bars, "device")
    assert bool((var >= 0).all())
    if case[0] == 1 or (case[0] == 2 and case[3] == "equal"):     # one sample; two equal ones (2p, 4p^2 / 2 are exact)
        assert bool((var == 0).all())
    three = ops.mc_cls_stats(x)                                                   # want_var=False: same statistics
    assert len(three) == 3 and all(_bits_equal(a, b) for a, b in zip(three, (mean_prob, ent, mi)))


MEAN_CASES = [(t, n) for t in (1, 2, 10) for n in (1, 300 * 8)] + [(2, BIG)]


def mean_case(t, n):
    x = torch.randn(t, n, generator=torch.Generator().manual_seed(t + n % 1000)) * 3 + 1
    # T - 1 additions of partial sums <= T max|x| and one division: <= T * 2^-24 * max|x|; 4x headroom over that bound
    return dict(x=x), dict(mean=x.double().mean(0)), dict(mean=4 * t * U / 2 * float(x.abs().max()))


def mean_restate(inp):
    s = torch.zeros_like(inp["x"][0])
    for row in inp["x"]:
        s = s + row
    return dict(mean=s / float(inp["x"].shape[0]))


@pytest.mark.parametrize("case", MEAN_CASES, ids=lambda c: "T%d-n%d" % c)
def test_cpu_restatement_mc_mean(case):
    inp, ref, bars = mean_case(*case)
    _check_all("mc_mean", "T%d-n%d" % case, mean_restate(inp), ref, bars, "cpu32", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MEAN_CASES, ids=lambda c: "T%d-n%d" % c)
def test_mc_mean(hip, case):
    inp, ref, bars = mean_case(*case)
    _check_all("mc_mean", "T%d-n%d" % case, dict(mean=_ops().mc_mean(inp["x"].to(DEV))), ref, bars, "device")


EXP_SIZES = [1, 300 * 8, BIG]


def exp_case(n):
    x = torch.rand(n, generator=torch.Generator().manual_seed(n % 1000)) * 175 - 87          # [-87, 88): normal results
    x[0] = -87.0
    x[-1] = 88.0
    ref = torch.exp(x.double())
    # relative error: a correctly rounded result is within 2^-24 = 5.96e-8, a 1-ulp expf within 2^-23 = 1.19e-7.  The
    # float32 restatement (torch.exp) measures 6.18e-8 over the 2097229 points; the bar is 4x that.
    return dict(x=x), dict(y=ref), dict(y=2.5e-7 * ref)


@pytest.mark.parametrize("n", EXP_SIZES)
def test_cpu_restatement_exp(n):
    inp, ref, bars = exp_case(n)
    _check_all("exp", "n%d" % n, dict(y=torch.exp(inp["x"])), ref, bars, "cpu32", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("n", EXP_SIZES)
def test_exp(hip, n):
    inp, ref, bars = exp_case(n)
    _check_all("exp", "n%d" % n, dict(y=_ops().exp(inp["x"].to(DEV))), ref, bars, "device")


# ================================================================================================
# 5. spatial_mean, spatial_mean_bwd, act_bwd
# ================================================================================================
SPATIAL_SHAPES = [(1, 1, 4), (37, 7, 2048), (5, 14, 36)]


@functools.lru_cache(maxsize=None)
def spatial_case(r, p, c):
    g = torch.Generator().manual_seed(r + p + c)
    x = torch.randn(r, p, p, c, generator=g)
    dout = torch.randn(r, c, generator=g)
    xd = x.double().requires_grad_(True)
    out = xd.permute(0, 3, 1, 2).mean(3).mean(2)
    out.backward(dout.double())
    # forward: P - 1 additions per row (partial sums <= P max|x|), a division, P - 1 additions of row means, a division:
    # <= (2P + 2) * 2^-24 * max|x| in all; backward: 1 / P^2 rounded once and one product: 2 * 2^-24 relative.  4x headroom.
    bars = dict(out=4 * (2 * p + 2) * U / 2 * float(x.abs().max()), dx=4 * 2 * U / 2 * float(dout.abs().max()) / (p * p))
    return dict(x=x, dout=dout, p=p), dict(out=out.detach(), dx=xd.grad), bars


def spatial_restate(inp):
    x, dout, p = inp["x"], inp["dout"], inp["p"]
    out = torch.zeros(x.shape[0], x.shape[3])
    for h in range(p):
        row = torch.zeros_like(out)
        for w in range(p):
            row = row + x[:, h, w]
        out = out + row / float(p)
    inv = np.float32(1.0) / (np.float32(p) * np.float32(p))
    return dict(out=out / float(p), dx=(dout * float(inv))[:, None, None, :].expand(-1, p, p, -1))


@pytest.mark.parametrize("shape", SPATIAL_SHAPES, ids=lambda s: "R%d-P%d-C%d" % s)
def test_cpu_restatement_spatial_mean(shape):
    inp, ref, bars = spatial_case(*shape)
    _check_all("spatial", "R%d-P%d-C%d" % shape, spatial_restate(inp), ref, bars, "cpu32", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SPATIAL_SHAPES, ids=lambda s: "R%d-P%d-C%d" % s)
def test_spatial_mean_fwd_bwd(hip, shape):
    ops = _ops()
    inp, ref, bars = spatial_case(*shape)
    got = dict(out=ops.spatial_mean(inp["x"].to(DEV)), dx=ops.spatial_mean_bwd(inp["dout"].to(DEV), inp["p"]))
    assert got["dx"].shape == inp["x"].shape
    _check_all("spatial", "R%d-P%d-C%d" % shape, got, ref, bars, "device")


def spatial_bwd_big_case():
    r, p, c = 300, 7, 2048                                           # R P^2 C / 4 = 7526400 > 8192 * 256
    dout = torch.randn(r, c, generator=torch.Generator().manual_seed(5))
    x = torch.zeros(r, c, p, p, dtype=torch.float64, requires_grad=True)
    x.mean(3).mean(2).backward(dout.double())
    return dout, p, x.grad.permute(0, 2, 3, 1), 4 * 2 * U / 2 * float(dout.abs().max()) / (p * p)


def test_cpu_restatement_spatial_mean_bwd_grid_stride():
    dout, p, ref, bar = spatial_bwd_big_case()
    got = spatial_restate(dict(x=torch.zeros(1, p, p, 4), dout=dout, p=p))["dx"]
    _check("spatial", "bwd-R300-P7-C2048", "dx", got, ref, bar, "cpu32", HEADROOM)


@pytest.mark.gpu
def test_spatial_mean_bwd_grid_stride_second_trip(hip):
    dout, p, ref, bar = spatial_bwd_big_case()
    assert ref.numel() // 4 > GRID_CAP
    _check("spatial", "bwd-R300-P7-C2048", "dx", _ops().spatial_mean_bwd(dout.to(DEV), p), ref, bar, "device")


ACT_SHAPES = [(131080, 64), (77, 4), (3 * 5 * 7, 64)]                 # rows * k / 4 = 2097280 > 8192 * 256; k = 4


def act_case(rows, k):
    g = torch.Generator().manual_seed(rows % 1000 + k)
    dy, y, sc = torch.randn(rows, k, generator=g), torch.randn(rows, k, generator=g), torch.rand(k, generator=g) + 0.5
    y.view(-1)[::7] = 0.0                                             # the mask is y > 0: neither zero passes
    y.view(-1)[3::7] = -0.0
    assert int((y == 0).sum()) >= 2 * (rows * k // 7) and bool(torch.signbit(y.view(-1)[3]))
    return dy, y, sc


def test_cpu_restatement_act_bwd_mask():
    """The expected value itself: a zero of either sign blocks the gradient, and masking by product equals selecting."""
    dy, y, sc = act_case(77, 4)
    mask = (y > 0).float()
    assert bool((mask.view(-1)[::7] == 0).all()) and bool((mask.view(-1)[3::7] == 0).all())
    assert torch.equal(dy * mask, torch.where(y > 0, dy, torch.zeros(())))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=lambda s: "rows%d-k%d" % s)
def test_act_bwd_edges(hip, shape):
    ops = _ops()
    dy, y, sc = act_case(*shape)
    assert shape[0] != 131080 or dy.numel() // 4 > GRID_CAP
    dconv, dres = ops.act_bwd(dy.to(DEV), y.to(DEV), sc.to(DEV), relu=True, want_res=True)
    mask = (y > 0).float()
    assert torch.equal(dres.cpu(), dy * mask) and torch.equal(dconv.cpu(), dy * mask * sc)      # bit-exact
    dconv, dres = ops.act_bwd(dy.to(DEV), y.to(DEV), None, relu=True)
    assert dres is None and torch.equal(dconv.cpu(), dy * mask)


# ================================================================================================
# 6. fpn_level_map
# ================================================================================================
LEVEL_PARAMS = [(2, 5), (3, 3), (2, 6)]          # FPN_POOL_LEVELS, one level only, and a k_max that shows 895 x 897


@functools.lru_cache(maxsize=None)
def level_boxes(n):
    """(n, 5) RoIs with integer corners: areas are exact in fp32 and fp64."""
    if n == 1:
        return torch.tensor([[0.0, 3, 4, 3 + 224, 4 + 224]])
    wh = []
    for s in (56, 112, 224, 448, 896):
        wh += [(s, s), (s, s + 1), (s, s - 1), (s + 1, s), (s - 1, s)]
    wh += [(895, 897),                # area 896^2 - 1: log2 falls 9e-7 short of level 6, only `+ eps` lifts it
           (0, 50), (50, 0), (0, 0),                                  # zero area: log2(0) = -inf -> k_min
           (-7, 30), (30, -7),                                        # negative area: sqrt -> NaN -> k_min (see below)
           (1, 1), (4000, 4000)]
    g = torch.Generator().manual_seed(6)
    fill = n - len(wh)
    rnd = torch.randint(1, 1500, (fill, 2), generator=g)
    wh = torch.cat((torch.tensor(wh), rnd)).float()
    xy = torch.randint(0, 200, (n, 2), generator=g).float()
    return torch.cat((torch.zeros(n, 1), xy, xy + wh), 1).contiguous()


def level_expected(rois, k_min, k_max):
    """O.fpn_level_map in float64, after checking that the oracle in float32 gives the same level on every box.
    Negative area: sqrt gives NaN, torch.clamp hands it through (lib/utils/torchpoolers.py:49-50) and the reference's
    .to(torch.int64) of it is not a level at all; the device's rule there is k_min (level 0), encoded here."""
    area = (rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2])
    ok = area >= 0
    want = O.fpn_level_map(rois.double(), k_min, k_max)
    assert torch.equal(want[ok], O.fpn_level_map(rois, k_min, k_max)[ok])
    want = torch.where(ok, want, torch.zeros_like(want))
    assert int(want.min()) >= 0 and int(want.max()) <= k_max - k_min
    return want


def level_restate(rois, k_min, k_max, s0=224.0, lvl0=4.0, eps=1e-6):
    area = (rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2])
    lvl = torch.floor(lvl0 + torch.log2((torch.sqrt(area) / s0).double()).float() + torch.tensor(eps))
    lvl = torch.where(lvl >= k_min, torch.clamp(lvl, max=float(k_max)), torch.tensor(float(k_min)))       # NaN -> k_min
    return lvl.long() - k_min


@pytest.mark.parametrize("n", [257, 1])
@pytest.mark.parametrize("k", LEVEL_PARAMS, ids=lambda k: "k%d-%d" % k)
def test_cpu_restatement_fpn_level_map(k, n):
    rois = level_boxes(n)
    want = level_expected(rois, *k)
    assert torch.equal(level_restate(rois, *k), want)
    if n > 1 and k == (2, 5):
        assert sorted(set(want.tolist())) == [0, 1, 2, 3]                        # every level is reached
    if n > 1 and k == (2, 6):                                                    # 895 x 897 needs `+ eps`
        i = 25
        assert tuple((rois[i, 3:] - rois[i, 1:3]).tolist()) == (895.0, 897.0) and int(want[i]) == 4
        assert int(torch.floor(4.0 + torch.log2(torch.sqrt(torch.tensor(895.0 * 897.0)) / 224.0))) == 5


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 1])
@pytest.mark.parametrize("k", LEVEL_PARAMS, ids=lambda k: "k%d-%d" % k)
def test_fpn_level_map(hip, k, n):
    rois = level_boxes(n)
    want = level_expected(rois, *k)
    got = _ops().fpn_level_map(rois.to(DEV), *k)
    assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), want), \
        [(rois[i].tolist(), int(got[i]), int(want[i])) for i in torch.nonzero(got.cpu().long() != want).view(-1)[:8]]
