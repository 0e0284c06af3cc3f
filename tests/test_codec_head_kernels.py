"""The box codec (csrc/boxes.hip: bbox_transform_inv, lidar_bbox_transform_inv, uncertainty_transform_inv, clip_boxes;
csrc/targets.hip: bbox_transform, lidar_bbox_transform, bbox_overlaps) and the fused detection tail (csrc/head.hip, both
forms) at their edges.  Every kernel is called directly through ops.py, or through the C ABI where ops.py hides an argument
(fc7 == NULL), and compared with

  * a float32 step-by-step restatement of its arithmetic in numpy (one correctly rounded IEEE operation per step; exp and
    the image encoder's log are float32(f(float64(v))) like the kernels'), BIT FOR BIT wherever the kernel consists of such
    steps only: the box-math translation units are built with -ffp-contract=off;
  * a float64 reference built from the oracle's own functions (O.bbox_transform(_inv), O.lidar_3d_bbox_transform(_inv),
    O.(lidar_3d_)uncertainty_transform_inv, O.clip_boxes, O.bbox_overlaps) and torch (F.linear, F.softmax), at the bars below.

Case builders return (inputs, float64 reference, bars).  The unmarked ``test_cpu_restatement_*`` tests hold the float32
restatement to the same bars with 4x headroom, so a bar only one device's rounding could meet, or inputs on which the
reference itself is unstable, fail without a GPU.  NaN and Inf are compared by position first (NaN against NaN, Inf against
the Inf of the same sign that the float64 reference rounds to in float32), then every finite element by value; no element is
left out.

Which case reaches which regime (case ids as pytest prints them):
  classes per box 1 / 2 / 9        kc1-* kc2-* kc9-*
  row stride 4 / 5                 *-ld4-* / *-ld5-* (a fifth column of junk travels along, un-sliced)
  scale none / 0.5 / 1.7           *-s0 / *-s0.5 / *-s1.7 (1.7: the quotient x / scale is inexact)
  stride loop, second trip         big-kc1-ld5-s1.7: n * kc = 2048 * 256 + 77 (the decoders and clip_boxes cap at 2048 blocks;
                                   the uncertainty kernel has no loop: there it checks the launch grid)
  degenerate boxes                 every case: rows r % 16 == 1 (x2 == x1), 2 (x2 < x1), 3 (sub-pixel), up to 4000 px
  exp() extremes                   every case: size deltas exactly 0, +-10, -104 (exp -> 0), +89 (exp -> inf), j % 11 in 0..3
  NaN hand-through                 every case: box row 5 (x1 = NaN) and delta row 7; NaN again after clip_boxes
  clip_boxes bounds                clip-zero_lo / clip-nonzero_lo: on, nextafter inside / outside each bound, +-inf, NaN
  variance input, exactly 0        uc *-var (input_is_variance, u = 0 at j % 11 == 0)
  encoders n / strides             n1-ld4x4, n255-ld5x8, n257-ld8x5, n70000-ld5x5 (launch grid); LiDAR gt rows are 7 / 8 wide
  encode -> decode round trip      test_round_trip_* (float64 first: the inputs are well-conditioned)
  bbox_overlaps                    edges: identical (1), disjoint (0), one pixel apart, shared edge, zero-area and
                                   negative-extent queries; n4097-k257-ld5x5: n * k just above 4096 * 256, both strides 5
  head C                           C4 (C/4 = 1 lane), C8, C252 (C/4 = 63 < 64), C260 (65: lane tail), C1024 (256), C2048
  head K / n_out                   image K2 K4 K12 (n_out 10 / 20 / 60), LiDAR K2 K4 K8 (16 / 32 / 64 = the limit)
  head P, R                        P1 P2 P7, R1 R37
  fc7 == NULL                      every head case (second launch through the C ABI; the other outputs must not change)
  saturated softmax                *-sat: one logit leads by > 104 -> probabilities exactly 1 and 0
  head rejections                  K13 (image), K9 (LiDAR), C6, C16324 (the smallest C % 4 == 0 over 64 KB of LDS)

Bars.  Bit for bit against the restatement: the three decoders, both uncertainty forms, clip_boxes (also against
torch.clamp), the image encoder, bbox_overlaps and every output of the head (its reductions have a fixed order: serial over
the window, lane partials in channel order, xor butterfly).  Against float64: decoded boxes rtol 3e-7 + atol 1e-4 px (the
existing codec test) with the atol multiplied by max(1, |centre term|, |half-size term|) of the element; the head's own bars
(fc7 2e-6, cls_score / cls_prob / bbox_pred 1e-5, tests/test_gpu_parity.py) multiplied by max(1, max |reference|), and for
pred_boxes the decoder's bar plus what a bbox_pred error of its bar moves the box by; bbox_overlaps 1e-6 (the existing test).
The uncertainty bar is 4x the first-order float32 rounding bound of the formula (see _uc_bar).  The encoders had no direct
test: their bars are 4x the measured error of the float32 restatement, listed in WIDENED next to the case.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import frcnn_oracle as O

DEV = "cuda:0"
U = 2.0 ** -23                       # fp32 machine epsilon
HEADROOM = 4.0
f32 = np.float32
DEC_CAP = 2048 * 256                 # decoders / clip_boxes: min(ceil(total / 256), 2048) blocks of 256, then stride
OVL_CAP = 4096 * 256                 # bbox_overlaps

# Bars the float32 restatement could not meet with 4x headroom.  None of these numbers comes from a device result.
#   encode*, round_trip (no earlier bar): (section, case id, tensor) -> (bar, measured max |restatement - float64|); the bar
#     is 4x the measured error rounded up to three digits.
#   decode*, head pred_boxes (element-wise bars, see the docstring): -> (factor on the bar, measured max of error / bar); the
#     factor is 4x the measured ratio rounded up.  What it pays for is conditioning, not the kernel: a size exp(d) * (x2 - x1 + 1)
#     at d = 10 carries three roundings (1.5 U against the 3e-7 / 4 = 0.6 U the headroom leaves), and x / 1.7 rounds the
#     corners of a box of -0.5 or 1.2 px at x ~ 2000 to 1e-4 px, 1e-4 of its size, before exp(10) multiplies it.  The device is
#     held to the restatement bit for bit in every one of these cases.
WIDENED = {
    ("encode", "n1-ld4x4", "targets"): (6.00e-07, 1.499e-07),
    ("encode", "n255-ld5x8", "targets"): (7.97e-06, 1.991e-06),
    ("encode", "n257-ld8x5", "targets"): (1.91e-05, 4.763e-06),
    ("encode", "n70000-ld5x5", "targets"): (2.90e-05, 7.242e-06),
    ("encode_lidar", "n1-ld4x7", "targets"): (5.15e-07, 1.287e-07),
    ("encode_lidar", "n255-ld5x8", "targets"): (4.75e-06, 1.186e-06),
    ("encode_lidar", "n257-ld8x7", "targets"): (7.04e-06, 1.758e-06),
    ("encode_lidar", "n70000-ld5x8", "targets"): (2.65e-05, 6.623e-06),
    ("round_trip", "image", "boxes"): (4.89e-04, 1.221e-04),
    ("round_trip", "lidar", "boxes"): (2.45e-04, 6.104e-05),
    ("decode_lidar", "kc1-ld4-s0", "boxes"): (1.36, 0.3376),
    ("decode_lidar", "kc1-ld4-s1.7", "boxes"): (198, 49.3403),
    ("decode_lidar", "kc1-ld5-s0", "boxes"): (1.36, 0.3376),
    ("decode_lidar", "kc1-ld5-s0.5", "boxes"): (1.25, 0.3111),
    ("decode_lidar", "kc1-ld5-s1.7", "boxes"): (198, 49.3403),
    ("decode_lidar", "kc2-ld4-s0", "boxes"): (1.1, 0.2727),
    ("decode_lidar", "kc2-ld4-s0.5", "boxes"): (1.09, 0.2705),
    ("decode_lidar", "kc2-ld4-s1.7", "boxes"): (3.83, 0.9565),
    ("decode_lidar", "kc2-ld5-s0", "boxes"): (1.31, 0.3254),
    ("decode_lidar", "kc2-ld5-s0.5", "boxes"): (1.31, 0.3254),
    ("decode_lidar", "kc2-ld5-s1.7", "boxes"): (2.26, 0.5626),
    ("decode_lidar", "kc9-ld4-s0", "boxes"): (1.36, 0.3376),
    ("decode_lidar", "kc9-ld4-s0.5", "boxes"): (1.64, 0.4096),
    ("decode", "kc9-ld4-s1.7", "boxes"): (9.75, 2.4356),
    ("decode_lidar", "kc9-ld4-s1.7", "boxes"): (990, 247.4041),
    ("decode_lidar", "kc9-ld5-s0", "boxes"): (1.36, 0.3376),
    ("decode_lidar", "kc9-ld5-s0.5", "boxes"): (1.36, 0.3376),
    ("decode", "kc9-ld5-s1.7", "boxes"): (1.98, 0.4944),
    ("decode_lidar", "kc9-ld5-s1.7", "boxes"): (990, 247.4041),
    ("decode", "big-kc1-ld5-s1.7", "boxes"): (9.75, 2.4363),
    ("decode_lidar", "big-kc1-ld5-s1.7", "boxes"): (3.16e+03, 788.2909),
    ("head", "lidar-R37-C252-K4-P7-normal", "pred_boxes"): (2.24, 0.5580),
    ("head", "lidar-R37-C260-K8-P7-normal", "pred_boxes"): (2.94, 0.7331),
    ("head", "lidar-R37-C1024-K2-P1-normal", "pred_boxes"): (2.15, 0.5372),
    ("head", "lidar-R37-C2048-K8-P7-normal", "pred_boxes"): (1.15, 0.2862),
    ("head", "lidar-R37-C252-K8-P2-sat", "pred_boxes"): (4.01, 1.0007),
}


def _ops():
    from faster_rcnn_pytorch_multimodal_amd import ops
    return ops


def _hip():
    from faster_rcnn_pytorch_multimodal_amd import _hip
    return _hip


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _np(t):
    return t.detach().cpu().numpy()


def _assert_bits(section, case, name, got, want):
    """NaN against NaN by position; every other element bit for bit (the sign of a zero included)."""
    got, want = np.ascontiguousarray(_np(got) if torch.is_tensor(got) else got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    assert got.shape == want.shape, (section, case, name, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s %s %s: NaN at %d positions, expected %d; first difference at flat index %d" % (
        section, case, name, gn.sum(), wn.sum(), int(np.flatnonzero(gn != wn)[0]))
    bad = np.flatnonzero((got.view(np.int32) != want.view(np.int32)).reshape(-1) & ~gn.reshape(-1))
    print("CHK|%s|bits|%s|%s|differing=%d of %d" % (section, case, name, bad.size, got.size))
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s %s %s: %d of %d elements differ from the float32 restatement; first at flat index %d: got %r, "
                             "expected %r" % (section, case, name, bad.size, got.size, i, got.reshape(-1)[i], want.reshape(-1)[i]))


def _assert_close(section, case, name, got, ref64, bar, side, headroom=1.0):
    """Non-finite elements by position and value against the float64 reference rounded to float32, the finite ones within
    ``bar`` (a number or an array shaped like the reference).  Prints the figure before it asserts."""
    wide = WIDENED.get((section, case, name))
    if wide is not None:
        bar = wide[0] if bar is None else np.asarray(bar, dtype=np.float64) * wide[0]
    assert bar is not None, "no bar for %s %s %s" % (section, case, name)
    got = np.asarray(_np(got) if torch.is_tensor(got) else got, dtype=np.float64).reshape(-1)
    ref64 = np.asarray(_np(ref64) if torch.is_tensor(ref64) else ref64, dtype=np.float64).reshape(-1)
    assert got.shape == ref64.shape, (section, case, name, got.shape, ref64.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        ref32 = ref64.astype(f32).astype(np.float64)
    odd = ~np.isfinite(ref32)
    assert np.array_equal(~np.isfinite(got), odd), "%s %s %s (%s): non-finite elements at other positions than the reference's" % (
        section, case, name, side)
    assert np.array_equal(np.isnan(got), np.isnan(ref32)) and np.array_equal(got[odd & ~np.isnan(ref32)],
                                                                              ref32[odd & ~np.isnan(ref32)]), \
        "%s %s %s (%s): NaN / Inf elements differ from the reference's" % (section, case, name, side)
    bar_a = np.broadcast_to(np.asarray(bar, dtype=np.float64).reshape(-1), got.shape)
    fin = ~odd
    err = np.abs(got[fin] - ref64[fin])
    ratio = float((err / bar_a[fin]).max()) if err.size else 0.0
    print("CHK|%s|%s|%s|%s|err=%.3e|ratio=%.4f|nonfinite=%d" % (section, side, case, name, float(err.max()) if err.size else 0.0,
                                                            ratio, int(odd.sum())))
    assert ratio * headroom <= 1.0, "%s %s %s (%s): max err %.3e is %.3f of its bar, allowed %.3f" % (
        section, case, name, side, float(err.max()), ratio, 1.0 / headroom)


# ================================================================================================
# float32 restatements (numpy: every operator below is one correctly rounded IEEE operation on float32 arrays)
# ================================================================================================
def _quiet(fn):
    @functools.wraps(fn)
    def run(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    return run


def exp32(v):
    return np.exp(v.astype(np.float64)).astype(f32)          # exp_f32 of csrc/box_math.h: rounded once from a double


def log32(v):
    return np.log(v.astype(np.float64)).astype(f32)


def _corners32(boxes, scale):
    b = np.asarray(boxes, dtype=f32)[:, :4]
    if scale is not None:
        b = b / f32(scale)
    return [b[:, i:i + 1] for i in range(4)]


@_quiet
def decode32(boxes, deltas, scale):
    """decode_box (csrc/box_math.h) for (n, >= 4) boxes and (n, 4 kc) deltas."""
    x1, y1, x2, y2 = _corners32(boxes, scale)
    d = np.asarray(deltas, dtype=f32).reshape(len(boxes), -1, 4)
    one, half = f32(1), f32(0.5)
    w, h = x2 - x1 + one, y2 - y1 + one
    diag = np.sqrt(w * w + h * h)
    cx, cy = x1 + half * w, y1 + half * h
    pcx, pcy = d[:, :, 0] * diag + cx, d[:, :, 1] * diag + cy
    pw, ph = exp32(d[:, :, 2]) * w, exp32(d[:, :, 3]) * h
    return np.stack((pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph), 2).reshape(len(boxes), -1)


@_quiet
def lidar_decode32(rois, anchors, deltas, scale):
    x1, y1, x2, y2 = _corners32(rois, scale)
    a = np.asarray(anchors, dtype=f32)
    d = np.asarray(deltas, dtype=f32).reshape(len(rois), -1, 7)
    one, two = f32(1), f32(2)
    ln, wd, ht = x2 - x1 + one, y2 - y1 + one, a[:, 5:6]
    cx, cy, cz = x1 + ln / two, y1 + wd / two, a[:, 2:3]
    diag = np.sqrt(ln * ln + wd * wd)
    parts = (d[:, :, 0] * diag + cx, d[:, :, 1] * diag + cy, d[:, :, 2] * ht + cz, exp32(d[:, :, 3]) * ln,
             exp32(d[:, :, 4]) * wd, exp32(d[:, :, 5]) * ht, d[:, :, 6])         # the heading is the raw delta
    return np.stack(parts, 2).reshape(len(rois), -1)


@_quiet
def uc32(rois, anchors, uc, scale, lidar, is_var):
    x1, y1, x2, y2 = _corners32(rois, scale)
    u = np.asarray(uc, dtype=f32).reshape(len(rois), -1, 7)
    if is_var:
        u = np.sqrt(u)
    one = f32(1)
    ln, wd = x2 - x1 + one, y2 - y1 + one
    ux, uy = u[:, :, 0] * ln, u[:, :, 1] * wd
    ul, uw = exp32(u[:, :, 3]) - one, exp32(u[:, :, 4]) - one
    if not lidar:
        parts = (ux, uy, ul, uw)
    else:
        ht = np.asarray(anchors, dtype=f32)[:, 5:6]
        parts = (ux, uy, u[:, :, 2] * ht, ul, uw, exp32(u[:, :, 5]) - one, u[:, :, 6])
    parts = [np.broadcast_to(p, ux.shape) for p in parts]
    return np.stack([p * p for p in parts], 2).reshape(len(rois), -1)


def clip32(boxes, info):
    """clampf of csrc/box_math.h: v < lo ? lo : (v > hi ? hi : v) - a NaN fails both tests and passes through."""
    info = np.asarray(info, dtype=f32)
    lo = np.array([info[0], info[2], info[0], info[2]], dtype=f32)
    hi = np.array([info[1] - f32(1), info[3] - f32(1), info[1] - f32(1), info[3] - f32(1)], dtype=f32)
    b = np.asarray(boxes, dtype=f32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        return np.where(b < lo, lo, np.where(b > hi, hi, b)).reshape(np.shape(boxes))


@_quiet
def encode32(ex, gt):
    ex, gt = np.asarray(ex, dtype=f32), np.asarray(gt, dtype=f32)
    one, half = f32(1), f32(0.5)
    ew, eh = ex[:, 2] - ex[:, 0] + one, ex[:, 3] - ex[:, 1] + one
    diag = np.sqrt(ew * ew + eh * eh)
    ecx, ecy = ex[:, 0] + half * ew, ex[:, 1] + half * eh
    gw, gh = gt[:, 2] - gt[:, 0] + one, gt[:, 3] - gt[:, 1] + one
    gcx, gcy = gt[:, 0] + half * gw, gt[:, 1] + half * gh
    return np.stack(((gcx - ecx) / diag, (gcy - ecy) / diag, log32(gw / ew), log32(gh / eh)), 1)


@_quiet
def lidar_encode32(rois, anchors, gt):
    """encode_box_lidar: the device takes logf (within 1 ulp, not correctly rounded), restated here with the correctly rounded
    float32 logarithm - this one is compared at a bar, not bit for bit."""
    r, a, g = np.asarray(rois, dtype=f32), np.asarray(anchors, dtype=f32), np.asarray(gt, dtype=f32)
    one, two = f32(1), f32(2)
    ln, wd, ht = r[:, 2] - r[:, 0] + one, r[:, 3] - r[:, 1] + one, a[:, 5]
    cx, cy, cz = r[:, 0] + ln / two, r[:, 1] + wd / two, a[:, 2]
    diag = np.sqrt(ln * ln + wd * wd)
    return np.stack(((g[:, 0] - cx) / diag, (g[:, 1] - cy) / diag, (g[:, 2] - cz) / ht, log32(g[:, 3] / ln), log32(g[:, 4] / wd),
                     log32(g[:, 5] / ht), g[:, 6]), 1)


@_quiet
def overlaps32(boxes, query):
    """iou_plus1 of csrc/targets.hip, operation by operation."""
    b, q = np.asarray(boxes, dtype=f32)[:, None, :4], np.asarray(query, dtype=f32)[None, :, :4]
    one, zero = f32(1), f32(0)
    aa = (b[..., 2] - b[..., 0] + one) * (b[..., 3] - b[..., 1] + one)
    ab = (q[..., 2] - q[..., 0] + one) * (q[..., 3] - q[..., 1] + one)
    iw = np.maximum(np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0]) + one, zero)
    ih = np.maximum(np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1]) + one, zero)
    ua = aa + ab - iw * ih
    return iw * ih / ua


# ================================================================================================
# 1. decoders, uncertainty forms, clip_boxes
# ================================================================================================
CODEC_CASES = [(37, kc, ld, s) for kc in (1, 2, 9) for ld in (4, 5) for s in (None, 0.5, 1.7)] + [(DEC_CAP + 77, 1, 5, 1.7)]
INFO = np.array([0, 1242, 0, 375, 0, 0, 1.0], dtype=f32)


def _codec_id(c):
    n, kc, ld, s = c
    return "%skc%d-ld%d-s%s" % ("big-" if n > 37 else "", kc, ld, "0" if s is None else repr(s))


def _rois(n, ld, g):
    """Boxes up to 4000 px; rows r % 16 == 1: x2 == x1 and y2 == y1, == 2: x2 < x1 and y2 < y1, == 3: sub-pixel; row 5: NaN.
    No box has a +1 size of exactly 0 (inf * 0 would be a NaN in float32 that float64 does not have)."""
    xy = torch.rand(n, 2, generator=g) * torch.tensor([3000.0, 2000.0])
    wh = torch.rand(n, 2, generator=g) * torch.tensor([1000.0, 2000.0])
    b = torch.cat((xy, xy + wh), 1)
    r = torch.arange(n)
    m = r % 16 == 1
    b[m, 2:] = b[m, :2]
    m = r % 16 == 2
    b[m, 2], b[m, 3] = b[m, 0] - 2.5, b[m, 1] - 7.0
    m = r % 16 == 3
    b[m, 2], b[m, 3] = b[m, 0] + 0.25, b[m, 1] + 0.125
    if n > 5:
        b[5, 0] = float("nan")
    out = torch.full((n, ld), 777.0)                        # whatever follows the four coordinates must not be read as one
    out[:, :4] = b
    return out


SIZE_SPECIALS = {0: (0.0, 0.0), 1: (10.0, -10.0), 2: (-104.0, 89.0), 3: (89.0, -104.0)}


def _deltas(n, kc, e, size_cols, g):
    d = torch.randn(n, kc, e, generator=g) * 0.5
    j = torch.arange(n * kc).view(n, kc)
    for r, (a, b) in SIZE_SPECIALS.items():
        m = j % 11 == r
        for q, col in enumerate(size_cols):
            d[:, :, col][m] = a if q % 2 == 0 else b
    d[min(7, n - 1), 0, 0] = float("nan")
    return d.view(n, kc * e).contiguous()


def _deltas64(deltas, e, size_cols):
    """The deltas in float64 for the oracle.  exp_f32 is a float32 function: above log(FLT_MAX) = 88.7228 its value is +inf,
    whatever the product with the box size would have been in float64 (exp(89) / 2 is a float32 number); the reference takes
    that value of the function, everything else in float64."""
    d = deltas.double().view(deltas.shape[0], -1, e).clone()
    for col in size_cols:
        d[:, :, col][d[:, :, col] > float(np.log(np.float64(np.finfo(f32).max)))] = float("inf")
    return d.view(deltas.shape[0], -1)


def _anchors3d(n, g):
    a = torch.randn(n, 7, generator=g) * 3
    a[:, 5] = torch.rand(n, generator=g) * 3 + 0.5          # heights
    return a.contiguous()


def _decode_bar(ref, stride, centre_cols=None):
    """rtol 3e-7, atol 1e-4 px x max(1, |centre term|, |half-size term|) of the element (image boxes: both terms from the
    reference's own corners)."""
    r = np.asarray(_np(ref), dtype=np.float64).reshape(len(ref), -1, stride)
    with np.errstate(all="ignore"):
        if centre_cols is None:
            c = np.stack(((r[..., 0] + r[..., 2]) / 2, (r[..., 1] + r[..., 3]) / 2) * 2, 2)
            hs = np.stack(((r[..., 2] - r[..., 0]) / 2, (r[..., 3] - r[..., 1]) / 2) * 2, 2)
            term = np.maximum(np.abs(c), np.abs(hs))
        else:
            term = np.broadcast_to(np.abs(centre_cols)[:, None, :], r.shape)
        term = np.where(np.isfinite(term), term, 1.0)
        bar = 3e-7 * np.abs(r) + 1e-4 * np.maximum(1.0, term)
    return np.where(np.isfinite(bar), bar, 1.0).reshape(len(ref), -1)


@functools.lru_cache(maxsize=None)
def decode_case(case):
    n, kc, ld, s = case
    g = torch.Generator().manual_seed(1000 + n % 1000 + 10 * kc + ld)
    boxes, deltas = _rois(n, ld, g), _deltas(n, kc, 4, (2, 3), g)
    ref = O.bbox_transform_inv(boxes[:, :4].double(), _deltas64(deltas, 4, (2, 3)), s)
    return dict(boxes=boxes, deltas=deltas, scale=s), ref, _decode_bar(ref, 4)


@functools.lru_cache(maxsize=None)
def lidar_decode_case(case):
    n, kc, ld, s = case
    g = torch.Generator().manual_seed(2000 + n % 1000 + 10 * kc + ld)
    rois, anc, deltas = _rois(n, ld, g), _anchors3d(n, g), _deltas(n, kc, 7, (3, 4, 5), g)
    ref = O.lidar_3d_bbox_transform_inv(rois[:, :4].double(), anc.double(), _deltas64(deltas, 7, (3, 4, 5)), s)
    b = rois[:, :4].double() / (s if s is not None else 1.0)
    centre = torch.stack((b[:, 0] + (b[:, 2] - b[:, 0] + 1) / 2, b[:, 1] + (b[:, 3] - b[:, 1] + 1) / 2, anc[:, 2].double()) +
                         (torch.zeros(n, dtype=torch.float64),) * 4, 1).numpy()
    return dict(rois=rois, anchors=anc, deltas=deltas, scale=s), ref, _decode_bar(ref, 7, centre)


def _uc_bar(rois, anchors, u_std, scale, lidar, is_var):
    """4 x the first-order float32 rounding bound of the formula (half an ulp, U / 2 relative, per operation; the second-
    order term of the final square is kept because a size term can be exactly 0):
      x / scale            e_x   = U/2 |x / scale|                                   (0 without a scale)
      len = x2 - x1 + 1    e_len = e_x1 + e_x2 + U/2 |x2 - x1| + U/2 |len|
      u = sqrt(v)          e_u   = U/2 |u|                                           (0 for a standard deviation)
      t = u * len          e_t   = |u| e_len + |len| e_u + U/2 |t|                   (z: len = the anchor height, exact)
      t = exp(u) - 1       e_t   = exp(u) (e_u + U/2) + U/2 |t|
      t = u                e_t   = e_u
      out = t * t          e     = 2 |t| e_t + e_t^2 + U/2 t^2
    plus 2^-126 for results that underflow."""
    h = U / 2
    b = np.asarray(_np(rois), dtype=np.float64)[:, :4]
    if scale is not None:
        b = b / scale
    e_x = h * np.abs(b) if scale is not None else np.zeros_like(b)
    u = np.asarray(_np(u_std), dtype=np.float64).reshape(len(b), -1, 7)
    e_u = h * np.abs(u) if is_var else np.zeros_like(u)
    with np.errstate(all="ignore"):
        def size(i0, i1):
            d = b[:, i1] - b[:, i0]
            ln = d + 1
            return ln[:, None], (e_x[:, i0] + e_x[:, i1] + h * np.abs(d) + h * np.abs(ln))[:, None]
        ln, e_ln = size(0, 2)
        wd, e_wd = size(1, 3)
        ht = np.asarray(_np(anchors), dtype=np.float64)[:, 5:6] if lidar else None

        def lin(q, s_, e_s):
            t = u[:, :, q] * s_
            return t, np.abs(u[:, :, q]) * e_s + np.abs(s_) * e_u[:, :, q] + h * np.abs(t)

        def expm1(q):
            ex = np.exp(u[:, :, q])
            t = ex - 1
            return t, ex * (e_u[:, :, q] + h) + h * np.abs(t)

        terms = [lin(0, ln, e_ln), lin(1, wd, e_wd)]
        if lidar:
            terms += [lin(2, ht, 0.0), expm1(3), expm1(4), expm1(5), (u[:, :, 6], e_u[:, :, 6])]
        else:
            terms += [expm1(3), expm1(4)]
        bars = [2 * np.abs(t) * e + e * e + h * t * t for t, e in terms]
        bar = HEADROOM * np.stack(bars, 2).reshape(len(b), -1) + 2.0 ** -126
    return np.where(np.isfinite(bar), bar, 1.0)


UC_FORMS = [("bev-std", False, False), ("bev-var", False, True), ("lidar-std", True, False), ("lidar-var", True, True)]


@functools.lru_cache(maxsize=None)
def uc_case(case, form):
    n, kc, ld, s = case
    _, lidar, is_var = form
    g = torch.Generator().manual_seed(3000 + n % 1000 + 10 * kc + ld + (100 if lidar else 0) + (200 if is_var else 0))
    rois, anc = _rois(n, ld, g), _anchors3d(n, g)
    u = torch.rand(n, kc, 7, generator=g) * 0.5
    if not is_var:
        u = u * (torch.randint(0, 2, (n, kc, 7), generator=g).float() * 2 - 1)       # a raw standard deviation may be negative
    j = torch.arange(n * kc).view(n, kc)
    for r, vals in ((0, (0.0, 0.0, 0.0)), (1, (10.0, 10.0, 10.0)), (2, (89.0, 0.0, 89.0)), (3, (-104.0, 89.0, -104.0))):
        m = j % 11 == r
        for q, col in enumerate((3, 4, 5)):
            u[:, :, col][m] = abs(vals[q]) if is_var else vals[q]
    m = j % 11 == 0
    u[:, :, 0][m] = 0.0
    u[min(7, n - 1), 0, 1] = float("nan")
    u = u.view(n, kc * 7)
    inp_u = (u * u).contiguous() if is_var else u.contiguous()                       # the variance is what the kernel is handed
    u_std = torch.sqrt(inp_u.double()) if is_var else inp_u.double()
    if lidar:
        ref = O.lidar_3d_uncertainty_transform_inv(rois[:, :4].double(), anc.double(), None, u_std, s)
    else:
        ref = O.uncertainty_transform_inv(rois[:, :4].double(), None, u_std, s)
    bar = _uc_bar(rois, anc, u_std, s, lidar, is_var)
    return dict(rois=rois, anchors=anc, uc=inp_u, scale=s, lidar=lidar, is_var=is_var), ref, bar


def _clip_values(lo, hi):
    lo, hi = f32(lo), f32(hi)
    inf = f32(np.inf)
    return [lo, np.nextafter(lo, -inf), np.nextafter(lo, inf), hi, np.nextafter(hi, inf), np.nextafter(hi, -inf), inf, -inf,
            f32(np.nan), f32(0.5) * (lo + hi), -f32(0.0), f32(1e30), f32(-1e30)]


@functools.lru_cache(maxsize=None)
def clip_case(name):
    info = {"zero_lo": [0, 1242, 0, 375], "nonzero_lo": [3.5, 1000.25, 7.0, 600.0]}[name]
    i32 = np.asarray(info, dtype=f32)
    xs, ys = _clip_values(i32[0], i32[1] - f32(1)), _clip_values(i32[2], i32[3] - f32(1))
    rows = [(xs[i], ys[j], xs[(i + 3) % len(xs)], ys[(j + 5) % len(ys)]) for i in range(len(xs)) for j in range(len(ys))]
    boxes = torch.tensor(np.array(rows + rows[:1], dtype=f32)).view(-1, 8)          # 13 * 13 + 1 boxes, two classes per row
    ref = O.clip_boxes(boxes.double(), info)
    return dict(boxes=boxes, info=info), ref


@pytest.mark.parametrize("case", CODEC_CASES, ids=_codec_id)
def test_cpu_restatement_decoders(case):
    cid = _codec_id(case)
    inp, ref, bar = decode_case(case)
    got = decode32(_np(inp["boxes"]), _np(inp["deltas"]), inp["scale"])
    _assert_close("decode", cid, "boxes", got, ref, bar, "cpu", HEADROOM)
    assert np.isnan(got).any() and np.isinf(got).any() and (got[:, 2::4] <= got[:, 0::4]).any()      # the regimes are there
    inp, ref, bar = lidar_decode_case(case)
    got = lidar_decode32(_np(inp["rois"]), _np(inp["anchors"]), _np(inp["deltas"]), inp["scale"])
    _assert_close("decode_lidar", cid, "boxes", got, ref, bar, "cpu", HEADROOM)
    assert np.isnan(got).any() and np.isinf(got).any() and (got == 0).any()


@pytest.mark.parametrize("form", UC_FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("case", CODEC_CASES, ids=_codec_id)
def test_cpu_restatement_uncertainty(case, form):
    inp, ref, bar = uc_case(case, form)
    got = uc32(_np(inp["rois"]), _np(inp["anchors"]), _np(inp["uc"]), inp["scale"], inp["lidar"], inp["is_var"])
    _assert_close("uc", _codec_id(case) + "-" + form[0], "var", got, ref, bar, "cpu", 1.0)   # the bar holds the 4x already
    assert np.isnan(got).any() and np.isinf(got).any() and (got == 0).any()


@pytest.mark.parametrize("name", ["zero_lo", "nonzero_lo"])
def test_cpu_restatement_clip_boxes(name):
    inp, ref = clip_case(name)
    got = clip32(_np(inp["boxes"]), inp["info"])
    _assert_bits("clip", name, "vs O.clip_boxes", got, _np(ref).astype(f32))
    i32 = np.asarray(inp["info"], dtype=f32)
    b = inp["boxes"].view(-1, 4)
    want = torch.stack((b[:, 0].clamp(float(i32[0]), float(i32[1] - f32(1))), b[:, 1].clamp(float(i32[2]), float(i32[3] - f32(1))),
                        b[:, 2].clamp(float(i32[0]), float(i32[1] - f32(1))), b[:, 3].clamp(float(i32[2]), float(i32[3] - f32(1)))), 1)
    _assert_bits("clip", name, "vs torch.clamp", got.reshape(-1, 4), _np(want))
    assert np.isnan(got).sum() == np.isnan(_np(inp["boxes"])).sum() > 0 and not np.isinf(got).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CODEC_CASES, ids=_codec_id)
def test_bbox_transform_inv_and_clip(hip, case):
    ops, cid = _ops(), _codec_id(case)
    inp, ref, bar = decode_case(case)
    got = ops.bbox_transform_inv(inp["boxes"].to(DEV), inp["deltas"].to(DEV), inp["scale"])
    want = decode32(_np(inp["boxes"]), _np(inp["deltas"]), inp["scale"])
    _assert_bits("decode", cid, "boxes", got, want)
    _assert_close("decode", cid, "boxes", got, ref, bar, "gpu")
    clipped = ops.clip_boxes(got, INFO)                       # a diverged regression stays visible: NaN in, NaN out
    _assert_bits("decode", cid, "clipped", clipped, clip32(want, INFO))
    _assert_bits("decode", cid, "clipped vs O.clip_boxes", clipped, _np(O.clip_boxes(_t(want).double(), INFO)).astype(f32))
    assert np.isnan(_np(clipped)).sum() == np.isnan(want).sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", CODEC_CASES, ids=_codec_id)
def test_lidar_bbox_transform_inv(hip, case):
    ops, cid = _ops(), _codec_id(case)
    inp, ref, bar = lidar_decode_case(case)
    got = ops.lidar_bbox_transform_inv(inp["rois"].to(DEV), inp["anchors"].to(DEV), inp["deltas"].to(DEV), inp["scale"])
    _assert_bits("decode_lidar", cid, "boxes", got, lidar_decode32(_np(inp["rois"]), _np(inp["anchors"]), _np(inp["deltas"]),
                                                                   inp["scale"]))
    _assert_close("decode_lidar", cid, "boxes", got, ref, bar, "gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("form", UC_FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("case", CODEC_CASES, ids=_codec_id)
def test_uncertainty_transform_inv(hip, case, form):
    ops, cid = _ops(), _codec_id(case) + "-" + form[0]
    inp, ref, bar = uc_case(case, form)
    got = ops.uncertainty_transform_inv(inp["rois"].to(DEV), inp["uc"].to(DEV), inp["anchors"].to(DEV) if inp["lidar"] else None,
                                        inp["scale"], lidar=inp["lidar"], input_is_variance=inp["is_var"])
    _assert_bits("uc", cid, "var", got, uc32(_np(inp["rois"]), _np(inp["anchors"]), _np(inp["uc"]), inp["scale"], inp["lidar"],
                                             inp["is_var"]))
    _assert_close("uc", cid, "var", got, ref, bar, "gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["zero_lo", "nonzero_lo"])
def test_clip_boxes_at_the_bounds(hip, name):
    inp, ref = clip_case(name)
    got = _ops().clip_boxes(inp["boxes"].to(DEV), inp["info"])
    _assert_bits("clip", name, "vs restatement", got, clip32(_np(inp["boxes"]), inp["info"]))
    _assert_bits("clip", name, "vs O.clip_boxes", got, _np(ref).astype(f32))


# ================================================================================================
# 2. encoders, round trip, overlaps
# ================================================================================================
ENC_CASES = [(1, 4, 4), (255, 5, 8), (257, 8, 5), (70000, 5, 5)]
ENC_LIDAR_CASES = [(1, 4, 7), (255, 5, 8), (257, 8, 7), (70000, 5, 8)]         # gt rows [xc,yc,zc,l,w,h,ry(,cls)]: 7 or 8 wide


def _enc_id(c):
    return "n%d-ld%dx%d" % c


def _plain_boxes(n, ld, g, lo=4.0, hi=400.0):
    xy = torch.rand(n, 2, generator=g) * 1500
    wh = torch.rand(n, 2, generator=g) * (hi - lo) + lo
    out = torch.full((n, ld), -555.0)
    out[:, :4] = torch.cat((xy, xy + wh), 1)
    return out


@functools.lru_cache(maxsize=None)
def encode_case(case):
    n, ex_ld, gt_ld = case
    g = torch.Generator().manual_seed(4000 + n + ex_ld)
    ex = _plain_boxes(n, ex_ld, g)
    gt = _plain_boxes(n, gt_ld, g)
    gt[:, :2] = ex[:, :2] + torch.randn(n, 2, generator=g) * 30                    # overlapping pairs, like sampled RoIs
    gt[:, 2:4] = gt[:, :2] + (ex[:, 2:4] - ex[:, :2]) * torch.exp(torch.randn(n, 2, generator=g) * 0.4)
    ref = O.bbox_transform(ex[:, :4].double(), gt[:, :4].double())
    return dict(ex=ex.contiguous(), gt=gt.contiguous()), ref


@functools.lru_cache(maxsize=None)
def encode_lidar_case(case):
    n, roi_ld, gt_ld = case
    g = torch.Generator().manual_seed(5000 + n + roi_ld)
    rois, anc = _plain_boxes(n, roi_ld, g), _anchors3d(n, g)
    gt = torch.full((n, gt_ld), 3.0)
    c = (rois[:, :2] + rois[:, 2:4]) / 2
    gt[:, 0:2] = c + torch.randn(n, 2, generator=g) * 20
    gt[:, 2] = anc[:, 2] + torch.randn(n, generator=g)
    gt[:, 3:5] = (rois[:, 2:4] - rois[:, :2] + 1) * torch.exp(torch.randn(n, 2, generator=g) * 0.4)
    gt[:, 5] = anc[:, 5] * torch.exp(torch.randn(n, generator=g) * 0.3)
    gt[:, 6] = torch.randn(n, generator=g)
    ref = O.lidar_3d_bbox_transform(rois[:, :4].double(), anc.double(), gt[:, :7].double())
    return dict(rois=rois.contiguous(), anchors=anc, gt=gt.contiguous()), ref


@pytest.mark.parametrize("case", ENC_CASES, ids=_enc_id)
def test_cpu_restatement_bbox_transform(case):
    inp, ref = encode_case(case)
    _assert_close("encode", _enc_id(case), "targets", encode32(_np(inp["ex"]), _np(inp["gt"])), ref, None, "cpu", HEADROOM)


@pytest.mark.parametrize("case", ENC_LIDAR_CASES, ids=_enc_id)
def test_cpu_restatement_lidar_bbox_transform(case):
    inp, ref = encode_lidar_case(case)
    got = lidar_encode32(_np(inp["rois"]), _np(inp["anchors"]), _np(inp["gt"]))
    _assert_close("encode_lidar", _enc_id(case), "targets", got, ref, None, "cpu", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ENC_CASES, ids=_enc_id)
def test_bbox_transform(hip, case):
    inp, ref = encode_case(case)
    got = _ops().bbox_transform(inp["ex"].to(DEV), inp["gt"].to(DEV))
    _assert_bits("encode", _enc_id(case), "targets", got, encode32(_np(inp["ex"]), _np(inp["gt"])))
    _assert_close("encode", _enc_id(case), "targets", got, ref, None, "gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ENC_LIDAR_CASES, ids=_enc_id)
def test_lidar_bbox_transform(hip, case):
    inp, ref = encode_lidar_case(case)
    got = _ops().lidar_bbox_transform(inp["rois"].to(DEV), inp["anchors"].to(DEV), inp["gt"].to(DEV))
    _assert_close("encode_lidar", _enc_id(case), "targets", got, ref, None, "gpu")
    want = lidar_encode32(_np(inp["rois"]), _np(inp["anchors"]), _np(inp["gt"]))
    for col in (0, 1, 2, 6):                                  # everything but the three logf columns is exact arithmetic
        _assert_bits("encode_lidar", _enc_id(case), "column %d" % col, _np(got)[:, col], want[:, col])


def _round_trip_inputs(kind):
    """The inputs and what the round trip must return: the LiDAR codec returns gt itself; the image decoder places x2 at
    cx + w / 2 with the +1 width and no -1 (lib/model/bbox_transform.py:99-103, decode_box), so the reference's own round
    trip returns [x1, y1, x2 + 1, y2 + 1] - checked against the oracle in float64 before anything else."""
    if kind == "image":
        inp, _ = encode_case((257, 8, 5))
        return inp, inp["gt"][:, :4] + torch.tensor([0.0, 0.0, 1.0, 1.0])
    inp, _ = encode_lidar_case((257, 8, 7))
    return inp, inp["gt"][:, :7]


@pytest.mark.parametrize("kind", ["image", "lidar"])
def test_cpu_restatement_round_trip(kind):
    """decode(encode(ex, gt)) returns gt (see _round_trip_inputs): in float64 to 1e-9 px, so the inputs are well-conditioned,
    and in float32 with 4x headroom under the bar the device is held to."""
    inp, gt = _round_trip_inputs(kind)
    if kind == "image":
        t64 = O.bbox_transform(inp["ex"][:, :4].double(), inp["gt"][:, :4].double())
        back64 = O.bbox_transform_inv(inp["ex"][:, :4].double(), t64)
        back32 = decode32(_np(inp["ex"]), encode32(_np(inp["ex"]), _np(inp["gt"])), None)
    else:
        t64 = O.lidar_3d_bbox_transform(inp["rois"][:, :4].double(), inp["anchors"].double(), inp["gt"][:, :7].double())
        back64 = O.lidar_3d_bbox_transform_inv(inp["rois"][:, :4].double(), inp["anchors"].double(), t64)
        back32 = lidar_decode32(_np(inp["rois"]), _np(inp["anchors"]), lidar_encode32(_np(inp["rois"]), _np(inp["anchors"]),
                                                                                      _np(inp["gt"])), None)
    assert float((back64 - gt.double()).abs().max()) <= 1e-9
    _assert_close("round_trip", kind, "boxes", back32, gt.double(), None, "cpu", HEADROOM)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["image", "lidar"])
def test_round_trip_decode_of_encode_returns_gt(hip, kind):
    ops = _ops()
    inp, gt = _round_trip_inputs(kind)
    if kind == "image":
        ex, g_ = inp["ex"].to(DEV), inp["gt"].to(DEV)
        back = ops.bbox_transform_inv(ex, ops.bbox_transform(ex, g_))
    else:
        rois, anc = inp["rois"].to(DEV), inp["anchors"].to(DEV)
        back = ops.lidar_bbox_transform_inv(rois, anc, ops.lidar_bbox_transform(rois, anc, inp["gt"].to(DEV)))
    _assert_close("round_trip", kind, "boxes", back, gt.double(), None, "gpu")


def _overlaps64(boxes, query):
    """O.bbox_overlaps casts to float32 itself; this is its text in float64 (test_cpu_restatement_bbox_overlaps ties the two)."""
    b, q = boxes.double(), query.double()
    ba = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    qa = (q[:, 2] - q[:, 0] + 1) * (q[:, 3] - q[:, 1] + 1)
    iw = (torch.min(b[:, 2:3], q[:, 2:3].t()) - torch.max(b[:, 0:1], q[:, 0:1].t()) + 1).clamp(min=0)
    ih = (torch.min(b[:, 3:4], q[:, 3:4].t()) - torch.max(b[:, 1:2], q[:, 1:2].t()) + 1).clamp(min=0)
    return iw * ih / (ba.view(-1, 1) + qa.view(1, -1) - iw * ih)


OVL_CASES = ["edges", "n4097-k257-ld5x5"]


@functools.lru_cache(maxsize=None)
def overlaps_case(name):
    if name == "edges":
        boxes = torch.tensor([[10.0, 20.0, 49.0, 59.0], [100.0, 100.0, 100.0, 100.0], [0.0, 0.0, 7.0, 3.0]])
        query = torch.tensor([[10.0, 20.0, 49.0, 59.0],       # identical to box 0: exactly 1
                              [300.0, 300.0, 320.0, 330.0],   # disjoint from all: exactly 0
                              [51.0, 20.0, 80.0, 59.0],       # one pixel apart from box 0 (x 49 | 51): 0
                              [50.0, 20.0, 80.0, 59.0],       # adjacent pixels (49 | 50): still 0 under the +1 convention
                              [49.0, 20.0, 80.0, 59.0],       # sharing the edge column x = 49: one column of overlap
                              [30.0, 30.0, 29.0, 40.0],       # zero area (x2 = x1 - 1)
                              [30.0, 30.0, 20.0, 40.0],       # negative extent
                              [100.0, 100.0, 100.0, 100.0]])  # one pixel, identical to box 1: exactly 1
        ref = _overlaps64(boxes, query)
        assert ref[0, 0] == 1 and ref[1, 7] == 1 and (ref[:, 1] == 0).all() and ref[0, 2] == 0 and ref[0, 3] == 0
        assert ref[0, 4] == 40.0 / (1600 + 32 * 40 - 40)
        return dict(boxes=boxes, query=query), ref
    g = torch.Generator().manual_seed(6000)
    boxes, query = _plain_boxes(4097, 5, g, 4.0, 600.0), _plain_boxes(257, 5, g, 4.0, 600.0)
    assert boxes.shape[0] * query.shape[0] > OVL_CAP
    return dict(boxes=boxes.contiguous(), query=query.contiguous()), _overlaps64(boxes[:, :4], query[:, :4])


@pytest.mark.parametrize("name", OVL_CASES)
def test_cpu_restatement_bbox_overlaps(name):
    inp, ref = overlaps_case(name)
    got = overlaps32(_np(inp["boxes"]), _np(inp["query"]))
    _assert_close("overlaps", name, "iou", got, ref, 1e-6, "cpu", HEADROOM)
    _assert_close("overlaps", name, "O.bbox_overlaps", O.bbox_overlaps(inp["boxes"][:, :4], inp["query"][:, :4]), ref, 1e-6, "cpu",
                  HEADROOM)
    if name == "edges":
        assert got[0, 0] == 1 and got[1, 7] == 1 and (got[:, 1] == 0).all() and got[0, 2] == 0 and got[0, 3] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", OVL_CASES)
def test_bbox_overlaps(hip, name):
    inp, ref = overlaps_case(name)
    got = _ops().bbox_overlaps(inp["boxes"].to(DEV), inp["query"].to(DEV))
    _assert_bits("overlaps", name, "iou", got, overlaps32(_np(inp["boxes"]), _np(inp["query"])))
    _assert_close("overlaps", name, "iou", got, ref, 1e-6, "gpu")


# ================================================================================================
# 3. head_fc_softmax_decode, both forms
# ================================================================================================
# (form, R, C, K, P, variant)
HEAD_CASES = [
    ("image", 1, 4, 2, 1, "normal"), ("image", 37, 8, 4, 2, "normal"), ("image", 37, 252, 12, 7, "normal"),
    ("image", 1, 260, 2, 7, "normal"), ("image", 37, 1024, 4, 2, "normal"), ("image", 37, 2048, 12, 7, "normal"),
    ("image", 37, 2048, 2, 1, "normal"), ("image", 37, 260, 4, 2, "sat"),
    ("lidar", 37, 4, 8, 1, "normal"), ("lidar", 1, 8, 2, 2, "normal"), ("lidar", 37, 252, 4, 7, "normal"),
    ("lidar", 37, 260, 8, 7, "normal"), ("lidar", 37, 1024, 2, 1, "normal"), ("lidar", 37, 2048, 8, 7, "normal"),
    ("lidar", 1, 2048, 4, 2, "normal"), ("lidar", 37, 252, 8, 2, "sat"),
]
HEAD_SCALE = 0.6
HEAD_NORM = {"image": ((0.1, 0.1, 0.2, 0.2), (0.03, -0.02, 0.05, -0.04)),
             "lidar": ((0.1, 0.1, 0.3, 0.2, 0.2, 0.25, 0.5), (0.03, -0.02, 0.1, 0.05, -0.04, 0.02, 0.3))}
HEAD_OUTPUTS = ("fc7", "cls_score", "cls_prob", "bbox_pred", "pred_boxes")


def _head_id(c):
    return "%s-R%d-C%d-K%d-P%d-%s" % c


@_quiet
def head32(x, wc, bc, wb, bb, rois, anchors, stds, means, scale):
    """head_fc_softmax_decode_kernel step by step: x (R,P,P,C) float32."""
    r_, p_, _, c_ = x.shape
    k = wc.shape[0]
    e = wb.shape[0] // k
    inv = f32(p_)
    tot = np.zeros((r_, c_), f32)
    for h in range(p_):                                       # mean over W inside each row, then over the P row means
        row = np.zeros((r_, c_), f32)
        for w in range(p_):
            row = row + x[:, h, w, :]
        tot = tot + row / inv
    fc7 = tot / inv
    c4 = c_ // 4
    a = fc7.reshape(r_, 1, c4, 4)
    wgt = np.concatenate((wc, wb), 0).reshape(1, k * (1 + e), c4, 4)
    t = ((a[..., 0] * wgt[..., 0] + a[..., 1] * wgt[..., 1]) + a[..., 2] * wgt[..., 2]) + a[..., 3] * wgt[..., 3]   # (R, O, C4)
    trips = (c4 + 63) // 64
    t = np.concatenate((t, np.zeros(t.shape[:2] + (trips * 64 - c4,), f32)), 2).reshape(r_, -1, trips, 64)
    acc = np.zeros(t.shape[:2] + (64,), f32)
    for j in range(trips):                                    # lane l owns channels l, l + 64, ... (idle lanes add +0: exact)
        acc = acc + t[:, :, j, :]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):                          # acc += __shfl_xor(acc, off)
        acc = acc + acc[:, :, lanes ^ off]
    out = acc[:, :, 0] + np.concatenate((bc, bb))[None, :]
    score, raw = out[:, :k], out[:, k:]
    m = score.max(1, keepdims=True)
    ex = exp32(score - m)
    s = np.zeros((r_, 1), f32)
    for q in range(k):
        s = s + ex[:, q:q + 1]
    prob = ex / s
    d = raw.reshape(r_, k, e) * np.asarray(stds, f32) + np.asarray(means, f32)
    if e == 4:
        boxes = decode32(rois[:, 1:5], d.reshape(r_, -1), scale)
    else:
        boxes = lidar_decode32(rois[:, 1:5], anchors, d.reshape(r_, -1), scale)
    return dict(fc7=fc7, cls_score=score, cls_prob=prob, bbox_pred=raw, pred_boxes=boxes)


@functools.lru_cache(maxsize=None)
def head_case(case):
    form, r_, c_, k, p_, variant = case
    e = 4 if form == "image" else 7
    g = torch.Generator().manual_seed(7000 + HEAD_CASES.index(case))
    x = torch.randn(r_, p_, p_, c_, generator=g) + 0.3
    sc = 1.0 / np.sqrt(c_)
    wc, bc = torch.randn(k, c_, generator=g) * sc, torch.randn(k, generator=g) * 0.5
    wb, bb = torch.randn(e * k, c_, generator=g) * sc, torch.randn(e * k, generator=g) * 0.1
    if variant == "sat":
        bc[1] += 150.0                                        # class 1 leads by far more than 104: exp() of the rest is 0
    rois = torch.cat((torch.zeros(r_, 1), _plain_boxes(r_, 4, g, 4.0, 600.0)), 1).contiguous()
    anc = _anchors3d(r_, g)
    stds, means = HEAD_NORM[form]
    inp = dict(x=x, wc=wc, bc=bc, wb=wb, bb=bb, rois=rois, anchors=anc if e == 7 else None, stds=stds, means=means)
    fc7 = x.double().mean(2).mean(1)                          # NHWC: .mean(3).mean(2) of the reference's NCHW tensor
    score = F.linear(fc7, wc.double(), bc.double())
    prob = F.softmax(score, 1)
    raw = F.linear(fc7, wb.double(), bb.double())
    d = (raw.view(r_, k, e) * torch.tensor(stds, dtype=torch.float64) + torch.tensor(means, dtype=torch.float64)).view(r_, -1)
    b = rois[:, 1:5].double()
    if e == 4:
        boxes = O.bbox_transform_inv(b, d, HEAD_SCALE)
        dbar = _decode_bar(boxes, 4)
    else:
        boxes = O.lidar_3d_bbox_transform_inv(b, anc.double(), d, HEAD_SCALE)
        bs = b / HEAD_SCALE
        centre = torch.stack((bs[:, 0] + (bs[:, 2] - bs[:, 0] + 1) / 2, bs[:, 1] + (bs[:, 3] - bs[:, 1] + 1) / 2,
                              anc[:, 2].double()) + (torch.zeros(r_, dtype=torch.float64),) * 4, 1).numpy()
        dbar = _decode_bar(boxes, 7, centre)
    ref = dict(fc7=fc7, cls_score=score, cls_prob=prob, bbox_pred=raw, pred_boxes=boxes)
    big = lambda t_: max(1.0, float(t_.abs().max()))
    bars = dict(fc7=2e-6 * big(fc7), cls_score=1e-5 * big(score), cls_prob=1e-5, bbox_pred=1e-5 * big(raw))
    # pred_boxes: the decoder's bar plus the box movement of a bbox_pred error of its bar, |d box / d raw| x bar: a centre
    # moves by std x diagonal (LiDAR z: std x height), a size by std x the size itself (each image corner by half of it, added
    # to the centre's), the heading by std
    bs = b / HEAD_SCALE
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
    return inp, ref, bars


def _head_np(inp):
    return [None if inp[n] is None else _np(inp[n]) for n in ("x", "wc", "bc", "wb", "bb", "rois", "anchors")]


@pytest.mark.parametrize("case", HEAD_CASES, ids=_head_id)
def test_cpu_restatement_head(case):
    inp, ref, bars = head_case(case)
    got = head32(*_head_np(inp), inp["stds"], inp["means"], HEAD_SCALE)
    for name in HEAD_OUTPUTS:
        _assert_close("head", _head_id(case), name, got[name], ref[name], bars[name], "cpu", HEADROOM)
    if case[5] == "sat":
        assert (got["cls_prob"][:, 1] == 1).all() and (np.delete(got["cls_prob"], 1, 1) == 0).all()
        assert (_np(ref["cls_prob"]).astype(f32)[:, 1] == 1).all()


def _launch_head(lib, inp, form, want_fc7):
    """The C ABI directly: ops.head_fc_softmax_decode always passes an fc7 buffer."""
    H = _hip()
    dev = {n: (None if inp[n] is None else inp[n].to(DEV).contiguous()) for n in ("x", "wc", "bc", "wb", "bb", "rois", "anchors")}
    r_, p_, _, c_ = inp["x"].shape
    k = inp["wc"].shape[0]
    e = 4 if form == "image" else 7
    out = dict(fc7=torch.full((r_, c_), -7.0, device=DEV) if want_fc7 else None,
               cls_score=torch.full((r_, k), -7.0, device=DEV), cls_prob=torch.full((r_, k), -7.0, device=DEV),
               bbox_pred=torch.full((r_, e * k), -7.0, device=DEV), pred_boxes=torch.full((r_, e * k), -7.0, device=DEV))
    ptr = lambda t_: None if t_ is None else t_.data_ptr()
    head = [ptr(dev["x"]), r_, p_, c_, ptr(dev["wc"]), ptr(dev["bc"]), ptr(dev["wb"]), ptr(dev["bb"]), k, ptr(dev["rois"])]
    tail = [H.float_array(inp["stds"]), H.float_array(inp["means"]), HEAD_SCALE] + [ptr(out[n]) for n in HEAD_OUTPUTS] + [
        torch.cuda.current_stream().cuda_stream]
    if e == 4:
        rc = lib.frcnn_head_fc_softmax_decode(*(head + tail))
    else:
        rc = lib.frcnn_head_fc_softmax_decode_lidar(*(head + [ptr(dev["anchors"])] + tail))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.gpu
@pytest.mark.parametrize("case", HEAD_CASES, ids=_head_id)
def test_head_fc_softmax_decode_edges(hip, case):
    ops, cid, form = _ops(), _head_id(case), case[0]
    inp, ref, bars = head_case(case)
    out = ops.head_fc_softmax_decode(inp["x"].to(DEV), inp["wc"].to(DEV), inp["bc"].to(DEV), inp["wb"].to(DEV), inp["bb"].to(DEV),
                                     inp["rois"].to(DEV), list(inp["stds"]), list(inp["means"]), HEAD_SCALE,
                                     roi_anchors_3d=None if form == "image" else inp["anchors"].to(DEV))
    want = head32(*_head_np(inp), inp["stds"], inp["means"], HEAD_SCALE)
    for name in HEAD_OUTPUTS:
        _assert_close("head", cid, name, out[name], ref[name], bars[name], "gpu")
    for name in HEAD_OUTPUTS:
        _assert_bits("head", cid, name, out[name], want[name])
    # pred_boxes is the decode of the kernel's OWN bbox_pred, bit for bit
    k, e = case[3], 4 if form == "image" else 7
    own = _np(out["bbox_pred"]).reshape(-1, k, e) * np.asarray(inp["stds"], f32) + np.asarray(inp["means"], f32)
    rois = _np(inp["rois"])[:, 1:5]
    own_boxes = (decode32(rois, own.reshape(len(rois), -1), HEAD_SCALE) if e == 4 else
                 lidar_decode32(rois, _np(inp["anchors"]), own.reshape(len(rois), -1), HEAD_SCALE))
    _assert_bits("head", cid, "pred_boxes vs decode of own bbox_pred", out["pred_boxes"], own_boxes)
    if case[5] == "sat":
        prob = _np(out["cls_prob"])
        assert (prob[:, 1] == 1).all() and (np.delete(prob, 1, 1) == 0).all() and not np.isnan(prob).any()
    # fc7 == NULL: the same launch without the fc7 store; every other output identical
    rc, bare = _launch_head(hip, inp, form, want_fc7=False)
    assert rc == 0, _hip().load().frcnn_last_error()
    for name in HEAD_OUTPUTS[1:]:
        _assert_bits("head", cid, name + " with fc7 == NULL", bare[name], _np(out[name]))


HEAD_REJECTS = [("image", 13, 8, "classes"), ("lidar", 9, 8, "classes"), ("image", 2, 6, "c%4"), ("lidar", 2, 6, "c%4"),
                ("image", 2, 16324, "too large"), ("lidar", 2, 16324, "too large")]


@pytest.mark.gpu
@pytest.mark.parametrize("rej", HEAD_REJECTS, ids=lambda r: "%s-K%d-C%d" % r[:3])
def test_head_rejections(hip, rej):
    """K over the 64-output limit, C % 4 != 0 and C over the LDS limit: an error with a message and no launch (the outputs
    keep their fill).  C = 16320 is the largest that fits: (C + 64) floats = 64 KB."""
    form, k, c_, what = rej
    e = 4 if form == "image" else 7
    g = torch.Generator().manual_seed(5)
    inp = dict(x=torch.randn(2, 1, 1, c_, generator=g), wc=torch.randn(k, c_, generator=g), bc=torch.zeros(k),
               wb=torch.randn(e * k, c_, generator=g), bb=torch.zeros(e * k),
               rois=torch.tensor([[0.0, 1.0, 2.0, 30.0, 40.0]] * 2), anchors=_anchors3d(2, g) if e == 7 else None,
               stds=HEAD_NORM[form][0], means=HEAD_NORM[form][1])
    rc, out = _launch_head(hip, inp, form, want_fc7=True)
    msg = (hip.frcnn_last_error() or b"").decode()
    assert rc != 0 and "head_fc_softmax_decode" in msg and what in msg, (rc, msg)
    for name in HEAD_OUTPUTS:
        assert bool((out[name] == -7.0).all()), name
    with pytest.raises(_hip().HipError, match="head_fc_softmax_decode"):
        _ops().head_fc_softmax_decode(inp["x"].to(DEV), inp["wc"].to(DEV), inp["bc"].to(DEV), inp["wb"].to(DEV), inp["bb"].to(DEV),
                                      inp["rois"].to(DEV), list(inp["stds"]), list(inp["means"]), HEAD_SCALE,
                                      roi_anchors_3d=None if e == 4 else inp["anchors"].to(DEV))
