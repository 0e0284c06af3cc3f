"""The training-target kernels of csrc/targets.hip at their edges: frcnn_anchor_target_layer (atl_overlap / atl_label /
atl_mark_keep / atl_finalize) and frcnn_proposal_target_layer[_lidar] (ptl_kernel<4> / <7>).  Both are called directly through
ops.anchor_target_layer / ops.proposal_target_layer with thresholds, batch sizes and fractions as arguments (cfg is not
touched) and compared with a float64 numpy reference written here from the reference project's two layers
(lib/layer_utils/anchor_target_layer.py:22-165, proposal_target_layer.py:22-262).  A wrong training target raises no error,
training only goes worse - so everything that can be pinned is pinned.

Case builders return (inputs, reference, bars).  Boxes have integer coordinates and areas below 2^24, so an IoU is ONE
correctly rounded division of exact integers in float32 and in float64 alike; every builder asserts (``_assert_clear``) that no
overlap lies within 1e-6 of a threshold unless it equals it exactly (only with float32-representable thresholds: 0.25, 0.5,
0.75), and that two overlaps that compete in an argmax or for a gt's best are either equal or 1e-6 apart.  float32 and float64
then classify identically by construction; the unmarked ``test_cpu_restatement_*`` twins prove it for every case id the GPU
tests have: they restate the kernel's float32 arithmetic in its own order (IoU, labels, encoders with log in double on the
float32 ratio) and run oracle/frcnn_oracle.py's anchor_target_layer / proposal_target_layer / bbox_overlaps / bbox_transform /
lidar_3d_bbox_transform on the same inputs: the oracle's output must pass the very checks the device output has to pass.

The random draws are NOT replayed.  The contract is the reference's - a uniform random subset - and is tested four ways:
(1) everything that does not depend on the draw is compared exactly; (2) what depends on it by invariants: kept sets are
subsets of the unsampled candidate sets, counts hit the quotas exactly, weights are 1 / (kept fg + kept bg), every sampled RoI
row is a bit copy of a live unskipped candidate of the right kind and its score / assignment / 3-D anchor / targets belong to
that same row (RoI column 0 carries the row id); (3) the same seed gives the same bits, seed = s with seed_dev = [d] gives the
bits of seed = s + d (one pair wraps past 2^32, one has d >= 2^31), another seed gives another subset; (4) uniformity over
512 consecutive seeds (anchor layer) and over 256 draws with replacement (proposal layer), 6 sigma bands derived at the case.

Which case reaches which regime (case ids as pytest prints them).  Anchor target layer:
  anchor count                     n1 n255 n256 n257 n300 (one / two blocks of 256, the ragged last wave)
  n < rpn_batchsize (keep scan)    n1 n255 n225 (150 fg > 128) n100 (60 fg + 40 bg: all 100 kept), default 256 / 0.5, each run
                                   straight after a 300-anchor call so the workspace is not fresh: atl_mark_keep_kernel must stop
                                   at min(n, quota slots), what the sort wrote
  label kernel, second trip        big-label: n = 1024 * 256 + 300 (a 300-anchor pattern tiled)
  overlap / finalize second trip   big-overlap: n = 4096 * 256 + 300, g = 2, rpn_batchsize 256: also the multi-workgroup top-k
  box count, LDS / global maxima   g1 g2 g512 g513 at n = 2000 (rpn_batchsize 4096: no sub-sampling, and again fewer anchors than slots);
                                   every third gt's best overlap is 0.6 < pos_ov: only the tie rule labels it
  gt_count                         gtcount3 (8-row buffer, 5 dead rows covering the frame) gtcount8 gtcount9 (clamped) gtcount0 (-> 1)
  frame                            frame-edges (x_lo, y_lo != 0; x1 == x_lo, x2 == x_hi - 1 inside; x1 == x_lo - 1, x2 == x_hi outside; y
                                   likewise), frame-none (no anchor inside: all outputs finite and zero, labels -1, counts [0, 0])
  label rules                      rules: identical anchors tie a gt's best 0.5 < pos_ov (all 1); a gt's best 0.1 < neg_ov (1, not 0);
                                   a gt only an outside anchor touches (labels nothing); overlap == pos_ov 0.75 (1); == neg_ov 0.25
                                   (not 0); two boxes at equal overlap (the first: sign of dx)
  sub-sampling                     sub-neither sub-fgover sub-bgover sub-both sub-fgbelow-fit (bg quota grows to batch - fg and then
                                   fits) sub-fgbelow-over sub-exact (candidates == quotas) sub-off (rpn_batchsize 16385)
  uniformity                       uniform: 300 anchors, 12 fg / 48 bg candidates, rpn_batchsize 16, fg_fraction 0.25
Proposal target layer, every case as E4 (image) and E7 (LiDAR: anchors_3d (R,7), true_gt_boxes (G,8)):
  RoI count / npad                 R1 R2 R3 R1023 R1024 R1025 R2048 R2049 R4096 (80 KB of LDS, two sort passes per thread); R4097 rejected
  roi_count                        count-mid count-over (clamped) count-0 (neither)
  regimes                          mixed-fgover mixed-fgunder mixed-bgfew fgonly-many fgonly-5 (256 rows from 5: uniformity) bgonly-many
                                   bgonly-few neither-mid (all overlaps in [bg_hi, fg_thresh)) neither-low (all below bg_lo 0.25)
  thresholds at equality           equal: overlap == fg_thresh 0.75 is fg, == bg_hi 0.5 is not bg, == bg_lo 0.25 is bg
  skip_mask                        skip-some, skip-allfg (skipping removes every fg candidate: mixed becomes bg only)
  classes                          num_classes 4 everywhere (gt classes 1, 3, 0, 2; a class-0 gt gives label 0 and no targets), nc2
  first-maximum argmax             the fourth gt row repeats the first box with another class: every tie must take row 0
  other arguments                  noscores (roi_scores None -> 0), gtcount-live / gtcount-over / gtcount-0 (dead rows would turn the
                                   far rows into fg candidates), seeds (seed_dev)
  normalisation                    non-zero means and unequal stds in every case: (t - mean) / std

Bars, all named below.  Exact (bit for bit): labels, counts, inside / outside weights, RoI / score / 3-D anchor copies,
assignments, zeros.  ATL_BAR: anchor targets, the absolute 2e-6 of test_gpu_parity.py::
test_anchor_target_layer_against_reference_golden times max(1, max |reference|).  PTL_BAR: proposal targets, the absolute 2e-5
of test_gpu_parity.py::test_proposal_target_layer[_lidar]_against_reference_golden times max(1, max |reference|).  The float32
restatements meet both with 4x headroom.  SIGMAS = 6: the uniformity bands, derived next to the cases.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import frcnn_oracle as O

DEV = "cuda:0"
f32, f64 = np.float32, np.float64
HEADROOM = 4.0
GAP = 1e-6                           # no overlap this close to a threshold (or to a competing overlap) unless equal
EPS32 = float(np.finfo(np.float32).eps)
ATL_BAR = 2e-6                       # test_gpu_parity.py::test_anchor_target_layer_against_reference_golden, atol
PTL_BAR = 2e-5                       # test_gpu_parity.py::test_proposal_target_layer_against_reference_golden, atol
SIGMAS = 6.0
LABEL_TRIP = 1024 * 256              # atl_label_kernel: at most 1024 blocks of 256, then grid-stride
OVERLAP_TRIP = 4096 * 256            # atl_overlap_kernel / atl_finalize_kernel: at most 4096 blocks of 256


def _ops():
    from faster_rcnn_pytorch_multimodal_amd import ops
    return ops


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _assert_bits(section, case, name, got, want):
    got, want = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(want))
    assert got.shape == want.shape and got.dtype == want.dtype, (section, case, name, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        assert np.isfinite(got).all(), (section, case, name, "not finite")
        bad = np.flatnonzero((got.view(np.int32) != want.view(np.int32)).reshape(-1))
    else:
        bad = np.flatnonzero((got != want).reshape(-1))
    print("CHK|%s|bits|%s|%s|differing=%d of %d" % (section, case, name, bad.size, got.size))
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s %s %s: %d of %d elements differ; first at flat index %d: got %r, expected %r" % (
            section, case, name, bad.size, got.size, i, got.reshape(-1)[i], want.reshape(-1)[i]))


def _assert_close(section, case, name, got, ref, bar, side, headroom=1.0):
    """max |got - ref| / bar <= 1 / headroom, everything finite; prints the figure before it asserts."""
    got = np.asarray(_np(got), dtype=f64).reshape(-1)
    ref = np.asarray(_np(ref), dtype=f64).reshape(-1)
    assert got.shape == ref.shape, (section, case, name, got.shape, ref.shape)
    assert np.isfinite(ref).all() and np.isfinite(got).all(), (section, case, name, "not finite")
    err = np.abs(got - ref)
    ratio = float(err.max() / bar) if err.size else 0.0
    print("CHK|%s|%s|%s|%s|err=%.3e|bar=%.3e|ratio=%.4f" % (section, side, case, name, float(err.max()) if err.size else 0.0,
                                                          bar, ratio))
    assert ratio * headroom <= 1.0, "%s %s %s (%s): max err %.3e is %.3f of its bar %.3e, allowed %.3f" % (
        section, case, name, side, float(err.max()), ratio, bar, 1.0 / headroom)


def _big(a):
    a = np.asarray(a)
    return max(1.0, float(np.abs(a).max())) if a.size else 1.0


@contextlib.contextmanager
def _oracle_settings(**kw):
    """The oracle keeps the reference's config values as module constants; a case's own values for the length of one call."""
    old = {k: getattr(O, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(O, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(O, k, v)


# ================================================================================================
# float64 reference and float32 restatement of the arithmetic both layers share
# ================================================================================================
def iou64(a, b):
    """lib/utils/bbox.py:5-33 (+1 areas) in float64: exact integers, one rounded division."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    aa = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    ab = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    iw = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]) + 1, 0)
    ih = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]) + 1, 0)
    inter = iw * ih
    assert float(max(aa.max(), ab.max())) < 2 ** 24          # areas, intersections and unions are exact in float32 too
    return inter / (aa[:, None] + ab[None, :] - inter)


def iou32(a, b):
    """iou_plus1 of csrc/targets.hip, float32, its order of operations."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    one = f32(1)
    aa = ((a[:, 2] - a[:, 0] + one) * (a[:, 3] - a[:, 1] + one))[:, None]
    ab = ((b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one))[None, :]
    iw = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]) + one, f32(0))
    ih = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]) + one, f32(0))
    ua = aa + ab - iw * ih
    out = iw * ih / ua
    assert out.dtype == np.float32
    return out


def encode64(ex, gt):
    """bbox_transform (lib/model/bbox_transform.py:52-70) in float64."""
    ex, gt = np.asarray(ex, f64), np.asarray(gt, f64)
    ew, eh = ex[:, 2] - ex[:, 0] + 1, ex[:, 3] - ex[:, 1] + 1
    gw, gh = gt[:, 2] - gt[:, 0] + 1, gt[:, 3] - gt[:, 1] + 1
    diag = np.sqrt(ew * ew + eh * eh)
    return np.stack((((gt[:, 0] + 0.5 * gw) - (ex[:, 0] + 0.5 * ew)) / diag, ((gt[:, 1] + 0.5 * gh) - (ex[:, 1] + 0.5 * eh)) / diag,
                     np.log(gw / ew), np.log(gh / eh)), 1)


def encode32(ex, gt):
    """encode_box of csrc/targets.hip: float32 throughout, log in double on the float32 ratio."""
    ex, gt = np.asarray(ex, f32), np.asarray(gt, f32)
    one, half = f32(1), f32(0.5)
    ew, eh = ex[:, 2] - ex[:, 0] + one, ex[:, 3] - ex[:, 1] + one
    diag = np.sqrt(ew * ew + eh * eh)
    ecx, ecy = ex[:, 0] + half * ew, ex[:, 1] + half * eh
    gw, gh = gt[:, 2] - gt[:, 0] + one, gt[:, 3] - gt[:, 1] + one
    gcx, gcy = gt[:, 0] + half * gw, gt[:, 1] + half * gh
    out = np.stack(((gcx - ecx) / diag, (gcy - ecy) / diag, np.log((gw / ew).astype(f64)).astype(f32),
                    np.log((gh / eh).astype(f64)).astype(f32)), 1)
    assert out.dtype == np.float32
    return out


def encode_lidar64(roi, anc, gt7):
    """lidar_3d_bbox_transform (lib/model/bbox_transform.py:16-49) in float64."""
    roi, anc, gt7 = np.asarray(roi, f64), np.asarray(anc, f64), np.asarray(gt7, f64)
    ln, wd, ht = roi[:, 2] - roi[:, 0] + 1, roi[:, 3] - roi[:, 1] + 1, anc[:, 5]
    cx, cy, cz = roi[:, 0] + ln / 2, roi[:, 1] + wd / 2, anc[:, 2]
    diag = np.sqrt(ln * ln + wd * wd)
    return np.stack(((gt7[:, 0] - cx) / diag, (gt7[:, 1] - cy) / diag, (gt7[:, 2] - cz) / ht, np.log(gt7[:, 3] / ln),
                     np.log(gt7[:, 4] / wd), np.log(gt7[:, 5] / ht), gt7[:, 6]), 1)


def encode_lidar32(roi, anc, gt7):
    """encode_box_lidar of csrc/targets.hip: float32 throughout, logf."""
    roi, anc, gt7 = np.asarray(roi, f32), np.asarray(anc, f32), np.asarray(gt7, f32)
    one, two = f32(1), f32(2)
    ln, wd, ht = roi[:, 2] - roi[:, 0] + one, roi[:, 3] - roi[:, 1] + one, anc[:, 5]
    cx, cy, cz = roi[:, 0] + ln / two, roi[:, 1] + wd / two, anc[:, 2]
    diag = np.sqrt(ln * ln + wd * wd)
    out = np.stack(((gt7[:, 0] - cx) / diag, (gt7[:, 1] - cy) / diag, (gt7[:, 2] - cz) / ht, np.log(gt7[:, 3] / ln),
                    np.log(gt7[:, 4] / wd), np.log(gt7[:, 5] / ht), gt7[:, 6]), 1)
    assert out.dtype == np.float32
    return out


def _assert_clear(cid, ov, thresholds):
    """No overlap within GAP of a threshold, unless it EQUALS a threshold that float32 represents.  Returns the equalities."""
    equal = 0
    for t in thresholds:
        near = np.abs(ov - t) < GAP
        if float(f32(t)) == t:
            equal += int((ov == t).sum())
            near &= ov != t
        assert not near.any(), "%s: an overlap within %g of the threshold %r" % (cid, GAP, t)
    return equal


def _assert_no_near_ties(cid, ov, axis):
    """Along ``axis`` every overlap either equals the maximum or lies GAP below it (float32 then orders them the same)."""
    if ov.size == 0:
        return
    d = ov.max(axis, keepdims=True) - ov
    assert not ((d > 0) & (d < GAP)).any(), "%s: two competing overlaps closer than %g" % (cid, GAP)


def _sub(rng, gt, w_rng, h_rng):
    """An integer box inside the 100 x 100 box ``gt`` with width / height in the given ranges: IoU = w * h / 10000."""
    w, h = int(rng.integers(w_rng[0], w_rng[1] + 1)), int(rng.integers(h_rng[0], h_rng[1] + 1))
    x = int(gt[0]) + int(rng.integers(0, 100 - w + 1))
    y = int(gt[1]) + int(rng.integers(0, 100 - h + 1))
    return [x, y, x + w - 1, y + h - 1]


def _within_sigmas(counts, trials, p):
    """Binomial(trials, p) keep counts: every one within SIGMAS standard deviations of the mean."""
    mean, sigma = trials * p, (trials * p * (1.0 - p)) ** 0.5
    dev = float(np.abs(np.asarray(counts, f64) - mean).max()) / sigma
    print("CHK|uniform|trials=%d|p=%.4f|mean=%.1f|sigma=%.2f|worst=%.2f sigma" % (trials, p, mean, sigma, dev))
    return dev <= SIGMAS, dev


# ================================================================================================
# 1. anchor target layer
# ================================================================================================
ATL_INFO = (10.0, 1010.0, 20.0, 620.0)                       # x_lo, x_hi, y_lo, y_hi: x_lo, y_lo != 0
ATL_GTS = np.array([[100, 100, 199, 199, 1], [100, 400, 199, 499, 1]], f32)


def _far(rng):
    """Inside the frame, no overlap with any gt box of ATL_GTS / the g-cases' grid rows used with it."""
    w, h = int(rng.integers(10, 61)), int(rng.integers(10, 61))
    x, y = int(rng.integers(300, 940)), int(rng.integers(40, 550))
    return [x, y, x + w - 1, y + h - 1]


def _out(rng):
    """Overlaps the frame but fails exactly one of the four inside tests."""
    x_lo, x_hi, y_lo, y_hi = (int(v) for v in ATL_INFO)
    x, y, r, k = int(rng.integers(300, 900)), int(rng.integers(100, 500)), int(rng.integers(0, 6)), int(rng.integers(4))
    return [[x_lo - 1 - r, y, x_lo + 40, y + 30], [x_hi - 40, y, x_hi + r, y + 30], [x, y_lo - 1 - r, x + 30, y_lo + 40],
            [x, y_hi - 40, x + 30, y_hi + r]][k]


def _mix(seed, fg, far, low=0, mid=0, out=0, gts=ATL_GTS):
    """fg: IoU >= 0.76 with a gt (round robin over the gts), low: 0.0475..0.28, mid: 0.3325..0.65, far: 0, out: outside."""
    rng = np.random.default_rng(seed)
    rows = [_sub(rng, gts[i % len(gts)], (95, 100), (80, 100)) for i in range(fg)]
    rows += [_far(rng) for _ in range(far)]
    rows += [_sub(rng, gts[i % len(gts)], (95, 100), (5, 28)) for i in range(low)]
    rows += [_sub(rng, gts[i % len(gts)], (95, 100), (35, 65)) for i in range(mid)]
    rows += [_out(rng) for _ in range(out)]
    return np.asarray(rows, f32)[rng.permutation(len(rows))]


def _atl(anchors, gt=ATL_GTS, info=ATL_INFO, neg=0.3, pos=0.7, batch=256, frac=0.5, gt_count=None, expect=None, n_equal=0):
    return dict(anchors=np.ascontiguousarray(anchors, f32), gt=np.ascontiguousarray(gt, f32), info=info, neg=neg, pos=pos,
                batch=batch, frac=frac, gt_count=gt_count, expect=expect, n_equal=n_equal)


def _tile(pattern, n):
    return pattern[np.arange(n) % len(pattern)]


def _grid_gts(g):
    """g boxes of 20 x 20 on a 30-pixel grid, 32 per row, inside ATL_INFO; rows stay above y = 540."""
    j = np.arange(g)
    x0, y0 = 20 + 30 * (j % 32), 25 + 30 * (j // 32)
    return np.stack((x0, y0, x0 + 19, y0 + 19, np.ones(g)), 1).astype(f32)


def _g_case(g, n=2000):
    """Every gt has one best anchor: the box itself (IoU 1), or for every third the box shifted by 5 (IoU 300 / 500 = 0.6
    < pos_ov: only the tie rule labels it); a quarter-height box inside (IoU 0.2: bg with a positive overlap); the rest far."""
    rng = np.random.default_rng(40 + g)
    gts = _grid_gts(g)
    rows = []
    for j in range(g):
        b = gts[j, :4].copy()
        if j % 3 == 2:
            b[0] += 5
            b[2] += 5
        rows.append(list(b))
        if j % 2 == 0 and len(rows) < n - g:
            rows.append([gts[j, 0], gts[j, 1] + 8, gts[j, 2], gts[j, 1] + 11])
    while len(rows) < n:
        w, h = int(rng.integers(5, 40)), int(rng.integers(5, 25))
        x, y = int(rng.integers(20, 950)), int(rng.integers(560, 590))
        rows.append([x, y, x + w - 1, y + h - 1])
    a = np.asarray(rows, f32)[rng.permutation(n)]
    return _atl(a, gts, batch=4096, frac=0.5)


def _gtcount_case(count):
    """8-row gt buffer, 3 live rows; the 5 dead rows hold a box covering the whole frame: read, it becomes the assigned box
    of every anchor the live rows do not touch (their targets change) and its own best anchor, the 300 x 200 box that no live
    row touches, turns from bg to fg (labels and counts change)."""
    live = np.array([[100, 100, 199, 199, 1], [100, 400, 199, 499, 1], [300, 100, 399, 199, 1]], f32)
    dead = np.tile(np.array([[10, 20, 1009, 619, 1]], f32), (5, 1))
    anchors = np.concatenate((_mix(50, 30, 60, 20, 20, 6, gts=live), np.array([[400, 250, 699, 449]], f32)))
    return _atl(anchors, np.concatenate((live, dead)), gt_count=count)


def _frame_edges():
    x_lo, x_hi, y_lo, y_hi = ATL_INFO
    g = ATL_GTS
    edge = [[x_lo, 100, x_lo + 50, 150], [x_lo - 1, 100, x_lo + 50, 150],                  # x1 == x_lo inside, one less outside
            [x_hi - 51, 100, x_hi - 1, 150], [x_hi - 51, 100, x_hi, 150],                  # x2 == x_hi - 1 inside, x_hi outside
            [300, y_lo, 350, y_lo + 50], [300, y_lo - 1, 350, y_lo + 50],
            [300, y_hi - 51, 350, y_hi - 1], [300, y_hi - 51, 350, y_hi],
            [x_lo, y_lo, x_hi - 1, y_hi - 1], [x_lo, y_lo, x_hi, y_hi - 1],                  # the whole frame: inside, one wider: outside
            [0, 0, 5, 5], [99, 100, 199, 199]]
    # the gt boxes reach over the frame's left edge in this case: an outside anchor equal to a gt must label nothing
    gt = np.array([[5, 100, 104, 199, 1], g[1]], f32)
    a = np.concatenate((np.asarray(edge, f32), np.array([[5, 100, 104, 199], [10, 100, 104, 199]], f32), _mix(60, 8, 20, 6, 6, 6)))
    return _atl(a, gt)


def _rules():
    gt = np.array([[100, 100, 199, 199, 1],     # A: best 0.75 == pos_ov; another anchor at 0.25 == neg_ov
                   [300, 100, 399, 199, 1],     # B: three identical anchors tie its best 0.5
                   [500, 100, 599, 199, 1],     # C: best anchor 0.1 < neg_ov
                   [900, 300, 999, 399, 1],     # D: only an anchor outside the frame touches it
                   [100, 300, 199, 399, 1],     # E and F: one anchor overlaps both by 20 columns; E comes first
                   [260, 300, 359, 399, 1]], f32)
    a = [[100, 100, 199, 174], [100, 100, 199, 124], [100, 130, 199, 169],                  # A: 0.75 -> 1, 0.25 -> -1, 0.4 -> -1
         [300, 100, 399, 149], [300, 100, 399, 149], [300, 100, 399, 149], [300, 150, 399, 189],   # B: 0.5 x 3 -> 1, 0.4 -> -1
         [500, 100, 599, 109], [500, 150, 599, 154],                                        # C: 0.1 -> 1 (best), 0.05 -> 0
         [950, 300, 1049, 399],                                                             # D: x2 >= x_hi, outside
         [100, 300, 199, 399], [260, 300, 359, 399], [180, 300, 279, 399],                  # E, F themselves; the anchor between them
         [600, 450, 640, 480], [700, 450, 760, 500], [400, 500, 420, 520]]                  # far: 0
    return _atl(np.asarray(a, f32), gt, neg=0.25, pos=0.75, n_equal=2)


ATL_BUILDERS = {
    "n1": lambda: _atl(np.array([[100, 100, 199, 199]], f32), ATL_GTS[:1], expect=(1, 0)),
    "n255": lambda: _atl(_mix(1, 40, 150, 40, 20, 5), expect=(40, 190)),
    "n256": lambda: _atl(_mix(2, 40, 151, 40, 20, 5), expect=(40, 191)),
    "n257": lambda: _atl(_mix(3, 40, 152, 40, 20, 5), expect=(40, 192)),
    "n300": lambda: _atl(_mix(4, 40, 195, 40, 20, 5), expect=(40, 235)),
    "n225": lambda: _atl(_mix(5, 150, 50, 25), expect=(150, 75)),
    "n100": lambda: _atl(_mix(6, 60, 30, 10), expect=(60, 40)),
    "big-label": lambda: _atl(_tile(_mix(4, 40, 195, 40, 20, 5), LABEL_TRIP + 300)),
    "big-overlap": lambda: _atl(_tile(_mix(7, 40, 195, 40, 20, 5), OVERLAP_TRIP + 300)),
    "g1": lambda: _g_case(1), "g2": lambda: _g_case(2), "g512": lambda: _g_case(512), "g513": lambda: _g_case(513),
    "gtcount3": lambda: _gtcount_case(3), "gtcount8": lambda: _gtcount_case(8), "gtcount9": lambda: _gtcount_case(9),
    "gtcount0": lambda: _gtcount_case(0),
    "frame-edges": _frame_edges,
    "frame-none": lambda: _atl(np.asarray([_out(np.random.default_rng(70 + i)) for i in range(70)], f32), expect=(0, 0)),
    "rules": _rules,
    "sub-neither": lambda: _atl(_mix(10, 10, 20, 10, 8, 4), expect=(10, 30)),
    "sub-fgover": lambda: _atl(_mix(11, 40, 12, 8, 8, 4), batch=64, frac=0.25, expect=(40, 20)),
    "sub-bgover": lambda: _atl(_mix(12, 32, 70, 30, 8, 4), batch=64, frac=0.5, expect=(32, 100)),
    "sub-both": lambda: _atl(_mix(13, 40, 70, 30, 8, 4), batch=64, frac=0.25, expect=(40, 100)),
    "sub-fgbelow-fit": lambda: _atl(_mix(14, 10, 35, 15, 8, 4), batch=64, frac=0.5, expect=(10, 50)),
    "sub-fgbelow-over": lambda: _atl(_mix(15, 10, 70, 30, 8, 4), batch=64, frac=0.5, expect=(10, 100)),
    "sub-exact": lambda: _atl(_mix(16, 16, 30, 18, 8, 4), batch=64, frac=0.25, expect=(16, 48)),
    "sub-off": lambda: _atl(_mix(17, 40, 70, 30, 8, 4), batch=16385, frac=0.5, expect=(40, 100)),
    "uniform": lambda: _atl(_mix(18, 12, 30, 18, 200, 40), batch=16, frac=0.25, expect=(12, 48)),
}
ATL_CASES = list(ATL_BUILDERS)
ATL_STALE = ("n1", "n255", "n225", "n100")      # n < rpn_batchsize: run straight after a call on the 300-anchor case


def atl_reference(inp):
    """Labels before sub-sampling, candidate sets, quotas, weights and targets in float64 (anchor_target_layer.py:22-165)."""
    a, gt = inp["anchors"].astype(f64), inp["gt"].astype(f64)
    if inp["gt_count"] is not None:
        gt = gt[:max(1, min(len(gt), inp["gt_count"]))]           # the kernel's clamp: live rows, at least one
    n = len(a)
    x_lo, x_hi, y_lo, y_hi = inp["info"]
    inside = (a[:, 0] >= x_lo) & (a[:, 1] >= y_lo) & (a[:, 2] < x_hi) & (a[:, 3] < y_hi)
    ov = iou64(a, gt[:, :4])
    arg, mx = ov.argmax(1), ov.max(1)                             # first maximum
    tie = np.zeros(n, bool)
    if inside.any():
        gmax = np.maximum(ov[inside].max(0), EPS32)               # :62: a gt nobody overlaps ties nothing
        tie = (ov == gmax[None, :]).any(1)
    lab = np.full(n, -1.0)
    lab[inside & (mx < inp["neg"])] = 0
    lab[inside & tie] = 1
    lab[inside & (mx >= inp["pos"])] = 1
    cand_fg, cand_bg = lab == 1, lab == 0
    cap = int(inp["frac"] * inp["batch"])                         # exact: every fraction used here is a power of two
    keep_fg = min(int(cand_fg.sum()), cap)
    keep_bg = min(int(cand_bg.sum()), inp["batch"] - keep_fg)
    tgt = np.zeros((n, 4))
    tgt[inside] = encode64(a[inside], gt[arg[inside], :4])
    weight = f32(1) / f32(keep_fg + keep_bg) if keep_fg + keep_bg else f32(0)
    return dict(inside=inside, ov=ov, arg=arg, labels=lab.astype(f32), cand_fg=cand_fg, cand_bg=cand_bg, keep_fg=keep_fg,
                keep_bg=keep_bg, targets=tgt, weight=weight, gt=gt,
                sampled=keep_fg < int(cand_fg.sum()) or keep_bg < int(cand_bg.sum()))


@functools.lru_cache(maxsize=None)
def atl_case(cid):
    inp = ATL_BUILDERS[cid]()
    ref = atl_reference(inp)
    ovi = ref["ov"][ref["inside"]]
    assert _assert_clear(cid, ovi, (inp["neg"], inp["pos"])) == inp["n_equal"], cid
    _assert_no_near_ties(cid, ovi, 1)
    _assert_no_near_ties(cid, ovi, 0)
    if inp["expect"] is not None:
        assert (int(ref["cand_fg"].sum()), int(ref["cand_bg"].sum())) == inp["expect"], (cid, ref["cand_fg"].sum(), ref["cand_bg"].sum())
    return inp, ref, dict(targets=ATL_BAR * _big(ref["targets"]))


def atl_check(cid, out, side, headroom=1.0):
    """The invariants of one call's outputs (numpy, anchor order); ``counts`` may be missing (the oracle has none)."""
    inp, ref, bars = atl_case(cid)
    lab = out["labels"]
    n = len(lab)
    assert lab.dtype == np.float32 and np.isin(lab, (-1.0, 0.0, 1.0)).all(), (cid, side)
    if out.get("counts") is not None:                            # candidates BEFORE sub-sampling: exact
        assert list(out["counts"]) == [int(ref["cand_fg"].sum()), int(ref["cand_bg"].sum())], (cid, side, out["counts"])
    fg, bg = lab == 1, lab == 0
    assert not (fg & ~ref["cand_fg"]).any() and not (bg & ~ref["cand_bg"]).any(), (cid, side, "kept set is no subset")
    assert (int(fg.sum()), int(bg.sum())) == (ref["keep_fg"], ref["keep_bg"]), (cid, side, fg.sum(), bg.sum())
    if not ref["sampled"]:
        _assert_bits("atl", cid, "labels (%s)" % side, lab, ref["labels"])
    _assert_close("atl", cid, "targets", out["targets"], ref["targets"], bars["targets"], side, headroom)
    assert (out["targets"][~ref["inside"]] == 0).all(), (cid, side, "targets outside the frame")
    assert (lab[~ref["inside"]] == -1).all(), (cid, side, "labels outside the frame")
    ones = np.ones((1, 4), f32)
    _assert_bits("atl", cid, "inside weights (%s)" % side, out["inside"], fg[:, None].astype(f32) * ones)
    _assert_bits("atl", cid, "outside weights (%s)" % side, out["outside"], np.where(lab >= 0, ref["weight"], f32(0))[:, None] * ones)
    assert out["outside"].shape == (n, 4)


def _atl_oracle(inp, ref, seed):
    """oracle.anchor_target_layer on the case: one 'pixel' per anchor (A = 1, H = n, W = 1) keeps the anchor order."""
    n = len(inp["anchors"])
    with _oracle_settings(TRAIN_RPN_NEGATIVE_OVERLAP=inp["neg"], TRAIN_RPN_POSITIVE_OVERLAP=inp["pos"]):
        lab, tgt, inw, outw = O.anchor_target_layer(torch.from_numpy(ref["gt"].astype(f32)), inp["info"], torch.from_numpy(inp["anchors"]),
                                                    1, n, 1, rpn_batchsize=inp["batch"], fg_fraction=inp["frac"],
                                                    generator=torch.Generator().manual_seed(seed))
    return dict(labels=_np(lab).reshape(n).astype(f32), targets=_np(tgt).reshape(n, 4), inside=_np(inw).reshape(n, 4),
                outside=_np(outw).reshape(n, 4), counts=None)


@pytest.mark.parametrize("cid", ATL_CASES)
def test_cpu_restatement_anchor_target_layer(cid):
    inp, ref, bars = atl_case(cid)
    a, gt = inp["anchors"], ref["gt"].astype(f32)
    ins = ref["inside"]
    # float32 classifies like float64: the kernel's IoU, first-maximum argmax, per-gt maxima, tie rule and thresholds
    ov = iou32(a, gt[:, :4])
    arg = ov.argmax(1)
    lab = np.full(len(a), -1.0, f32)
    if ins.any():
        gmax = np.maximum(ov[ins].max(0), f32(EPS32))
        mx = ov.max(1)
        lab[ins & (mx < f32(inp["neg"]))] = 0
        lab[ins & (mx > 0) & (ov == gmax[None, :]).any(1)] = 1
        lab[ins & (mx >= f32(inp["pos"]))] = 1
    _assert_bits("atl", cid, "float32 labels before sub-sampling", lab, ref["labels"])
    assert np.array_equal(arg[ins], ref["arg"][ins]), cid
    assert not ins.any() or np.array_equal(_np(O.bbox_overlaps(a[ins], gt[:, :4])), ov[ins]), cid
    tgt = np.zeros((len(a), 4), f32)
    tgt[ins] = encode32(a[ins], gt[arg[ins], :4])
    _assert_close("atl", cid, "targets", tgt, ref["targets"], bars["targets"], "restated", HEADROOM)
    if ins.any():
        _assert_close("atl", cid, "targets", _np(O.bbox_transform(torch.from_numpy(a[ins]).double(),
                                                                  torch.from_numpy(gt[arg[ins], :4]).double())),
                      ref["targets"][ins], 1e-12 * _big(ref["targets"]), "oracle float64")
        atl_check(cid, _atl_oracle(inp, ref, 3), "oracle")        # the reference's own draw passes the device's checks
    else:
        assert ref["keep_fg"] + ref["keep_bg"] == 0 and not ref["labels"].max() > -1    # the reference cannot run on an empty frame
    if inp["gt_count"] is not None and inp["gt_count"] < len(inp["gt"]):                # the dead rows matter: read, labels change
        wide = atl_reference(dict(inp, gt_count=None))
        assert not np.array_equal(wide["labels"], ref["labels"]) and not np.array_equal(wide["arg"], ref["arg"]), cid
    if cid == "rules":
        by = {tuple(int(v) for v in r): i for i, r in enumerate(a)}
        between = by[(180, 300, 279, 399)]
        assert ref["arg"][between] == 4 and ref["targets"][between, 0] < 0 and ref["labels"][between] == 0
        assert list(ref["labels"][:10]) == [1, -1, -1, 1, 1, 1, -1, 1, 0, -1]
    if cid in ("g1", "g2", "g512", "g513"):
        best = ref["ov"].argmax(0)
        assert (ref["labels"][best] == 1).all() and (ref["ov"].max(0) < inp["pos"]).sum() >= len(ref["gt"]) // 3, cid


def _atl_run(inp, seed, seed_dev=None, gt_count="case"):
    cnt = inp["gt_count"] if gt_count == "case" else gt_count
    cnt_dev = None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device=DEV)
    sd = None if seed_dev is None else torch.tensor([seed_dev - (1 << 32) if seed_dev >= (1 << 31) else seed_dev], dtype=torch.int32,
                                                    device=DEV)
    lab, tgt, inw, outw, counts = _ops().anchor_target_layer(torch.from_numpy(inp["anchors"]).to(DEV), torch.from_numpy(inp["gt"]).to(DEV),
                                                             inp["info"], inp["batch"], inp["frac"], inp["neg"], inp["pos"], seed,
                                                             seed_dev=sd, gt_count=cnt_dev)
    return dict(labels=_np(lab), targets=_np(tgt), inside=_np(inw), outside=_np(outw), counts=_np(counts))


def _same_bits(section, cid, name, a, b):
    for k in a:
        _assert_bits(section, cid, "%s: %s" % (name, k), a[k], b[k])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ATL_CASES)
def test_anchor_target_layer(hip, cid):
    inp, ref, _ = atl_case(cid)
    if cid in ATL_STALE:
        _atl_run(atl_case("n300")[0], 1)                         # the workspace this call frees is the next call's
    out = _atl_run(inp, 7)
    atl_check(cid, out, "device")
    assert np.isfinite(out["targets"]).all() and np.isfinite(out["outside"]).all()
    if cid == "frame-none":
        assert list(out["counts"]) == [0, 0] and (out["labels"] == -1).all()
        assert not out["targets"].any() and not out["inside"].any() and not out["outside"].any()
    if cid == "n100":
        assert (out["labels"] >= 0).all()
    if inp["gt_count"] is not None:                              # bit for bit the call on the clamped number of rows
        rows = max(1, min(len(inp["gt"]), inp["gt_count"]))
        _same_bits("atl", cid, "gt_count vs %d rows" % rows, out, _atl_run(dict(inp, gt=inp["gt"][:rows].copy()), 7, gt_count=None))


SEED_PAIRS = {"small": (5, 7), "wrap": (0xFFFFFFF0, 0x20), "high-d": (0x7FFFFFFF, 0x90000000)}


@pytest.mark.parametrize("pair", list(SEED_PAIRS))
def test_cpu_restatement_anchor_target_layer_seeds(pair):
    """What the GPU twin relies on: the sum is taken modulo 2^32 (uint32 `seed += *seed_dev`), and the case leaves the draw
    a choice: C(12, 4) * C(48, 12) subsets, so two seeds agree by chance with probability below 1e-12."""
    s, d = SEED_PAIRS[pair]
    assert 0 <= (s + d) & 0xFFFFFFFF < 2 ** 32 and ((s + d) >= 2 ** 32) == (pair != "small")
    _, ref, _ = atl_case("uniform")
    assert ref["sampled"] and (ref["keep_fg"], ref["keep_bg"]) == (4, 12)
    a = _atl_oracle(atl_case("uniform")[0], ref, 1)["labels"]
    b = _atl_oracle(atl_case("uniform")[0], ref, 2)["labels"]
    assert not np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(SEED_PAIRS))
def test_anchor_target_layer_seeds(hip, pair):
    inp, _, _ = atl_case("uniform")
    s, d = SEED_PAIRS[pair]
    total = (s + d) & 0xFFFFFFFF
    one = _atl_run(inp, total)
    _same_bits("atl", pair, "same seed", one, _atl_run(inp, total))
    _same_bits("atl", pair, "seed + seed_dev", one, _atl_run(inp, s, seed_dev=d))
    assert not np.array_equal(one["labels"], _atl_run(inp, (total + 1) & 0xFFFFFFFF)["labels"])
    atl_check("uniform", one, "device")


# Uniformity.  12 fg candidates of which 4 are kept, 48 bg candidates of which 12 are kept, 512 consecutive seeds: a
# candidate's keep count is Binomial(512, 1/3) (mean 170.7, sigma 10.67: 6 sigma = 64) or Binomial(512, 1/4) (mean 128,
# sigma 9.80: 6 sigma = 58.8) under a uniform subset.  P(|z| > 6) = 2e-9 per candidate, below 1.2e-7 over all 60 (the normal
# tail understates a binomial's by less than a factor of 4 this far out): a condition, not a measurement.
UNIFORM_SEEDS = 512


def _atl_uniformity(label_rows):
    _, ref, _ = atl_case("uniform")
    lab = np.stack(label_rows)
    assert lab.shape[0] == UNIFORM_SEEDS
    assert ((lab == 1).sum(1) == 4).all() and ((lab == 0).sum(1) == 12).all()
    assert not (lab == 1)[:, ~ref["cand_fg"]].any() and not (lab == 0)[:, ~ref["cand_bg"]].any()
    ok_fg, dev_fg = _within_sigmas((lab == 1).sum(0)[ref["cand_fg"]], UNIFORM_SEEDS, 4.0 / 12.0)
    ok_bg, dev_bg = _within_sigmas((lab == 0).sum(0)[ref["cand_bg"]], UNIFORM_SEEDS, 12.0 / 48.0)
    assert ok_fg and ok_bg, "keep counts up to %.2f (fg) / %.2f (bg) sigma from their binomial mean" % (dev_fg, dev_bg)


def test_cpu_restatement_anchor_target_layer_uniformity():
    """The same criterion on the reference's own method (torch.randperm, through the oracle)."""
    inp, ref, _ = atl_case("uniform")
    gen = torch.Generator().manual_seed(1234)
    gt, anchors = torch.from_numpy(ref["gt"].astype(f32)), torch.from_numpy(inp["anchors"])
    rows = [_np(O.anchor_target_layer(gt, inp["info"], anchors, 1, len(anchors), 1, rpn_batchsize=16, fg_fraction=0.25,
                                      generator=gen)[0]).reshape(-1) for _ in range(UNIFORM_SEEDS)]
    _atl_uniformity(rows)


@pytest.mark.gpu
def test_anchor_target_layer_uniformity(hip):
    inp, _, _ = atl_case("uniform")
    anchors, gt = torch.from_numpy(inp["anchors"]).to(DEV), torch.from_numpy(inp["gt"]).to(DEV)
    labs = [_ops().anchor_target_layer(anchors, gt, inp["info"], 16, 0.25, inp["neg"], inp["pos"], 1000 + s)[0]
            for s in range(UNIFORM_SEEDS)]
    _atl_uniformity(list(_np(torch.stack(labs))))


# ================================================================================================
# 2. proposal target layer
# ================================================================================================
PTL_TH = (0.75, 0.5, 0.25)                                   # fg_thresh, bg_hi, bg_lo: float32 represents all three
PTL_BOXES = np.array([[100, 100, 199, 199], [400, 100, 499, 199], [100, 400, 199, 499], [100, 100, 199, 199]], f32)
PTL_CLASSES = {4: (1, 3, 0, 2), 2: (1, 1, 0, 1)}             # row 2 is a class-0 box, row 3 repeats row 0's box: ties take row 0
PTL_GHOST = np.array([600, 400, 699, 499], f32)              # where the far rows sit; a dead gt row holds this box
PTL_MEANS = (0.1, -0.2, 0.3, 0.05, -0.15, 0.25, 0.4)
PTL_STDS = (0.1, 0.2, 0.3, 0.4, 0.15, 0.25, 0.5)
# kinds of RoI rows, by their overlap with their gt box (w * h / 10000 inside a 100 x 100 box)
KIND_RANGES = {"F": ((95, 100), (82, 100)),                  # 0.779 .. 1     fg
               "M": ((95, 100), (56, 73)),                   # 0.532 .. 0.73  neither
               "B": ((95, 100), (28, 48))}                   # 0.266 .. 0.48  bg


def _ptl(seed, comp, rows=64, frac=0.25, th=PTL_TH, num_classes=4, roi_count=None, skip=None, scores=True, dead=0, gt_count=None,
         uniform5=False):
    """comp: kind -> number of rows; "L" rows overlap nothing live (they sit in PTL_GHOST), "=0.75" / "=0.5" / "=0.25" rows
    have exactly that overlap.  Column 0 of a RoI is its row id."""
    rng = np.random.default_rng(seed)
    boxes, kinds = [], []
    for kind, count in comp.items():
        for _ in range(count):
            gt = PTL_BOXES[int(rng.integers(3))]
            if kind == "L":
                boxes.append(_sub(rng, PTL_GHOST, *KIND_RANGES["F"]))
            elif kind.startswith("="):
                h = int(round(float(kind[1:]) * 100))
                y = int(gt[1]) + int(rng.integers(0, 100 - h + 1))
                boxes.append([gt[0], y, gt[2], y + h - 1])
            else:
                boxes.append(_sub(rng, gt, *KIND_RANGES[kind]))
            kinds.append(kind)
    perm = rng.permutation(len(boxes))
    boxes, kinds = np.asarray(boxes, f32)[perm], np.asarray(kinds)[perm]
    r = len(boxes)
    rois = np.concatenate((np.arange(r, dtype=f32)[:, None], boxes), 1)
    g = len(PTL_BOXES) + dead
    gt = np.zeros((g, 5), f32)
    gt[:4, :4], gt[:4, 4] = PTL_BOXES, PTL_CLASSES[num_classes]
    gt[4:, :4], gt[4:, 4] = PTL_GHOST, 1
    true_gt = np.concatenate((rng.uniform(-20, 60, (g, 3)), rng.uniform(1.5, 12, (g, 3)), rng.uniform(-3.1, 3.1, (g, 1)), gt[:, 4:5]),
                             1).astype(f32)
    a3 = np.concatenate((rng.uniform(-20, 60, (r, 3)), rng.uniform(1.5, 12, (r, 3)), rng.uniform(-3.1, 3.1, (r, 1))), 1).astype(f32)
    mask = None
    if skip == "some":
        mask = (rng.uniform(size=r) < 0.3).astype(np.uint8)
    elif skip == "allfg":
        mask = np.isin(kinds, ("F", "=0.75")).astype(np.uint8)
    return dict(rois=rois, kinds=kinds, gt=gt, true_gt=true_gt, anchors_3d=a3, rows=rows, frac=frac, th=th, num_classes=num_classes,
                roi_count=roi_count, skip=mask, scores=(rng.uniform(0.05, 1.0, r).astype(f32) if scores else None), gt_count=gt_count,
                uniform5=uniform5)


def _sized(r):
    if r <= 3:
        return {1: dict(F=1), 2: dict(F=1, B=1), 3: dict(F=1, B=1, M=1)}[r]
    f, b, m = r // 8, r // 2, r // 8
    return dict(F=f, B=b, M=m, L=r - f - b - m)


PTL_BUILDERS = {("R%d" % r): (lambda r=r: _ptl(100 + r, _sized(r))) for r in (1, 2, 3, 1023, 1024, 1025, 2048, 2049, 4096)}
PTL_BUILDERS.update({
    "count-mid": lambda: _ptl(201, dict(F=40, B=200, M=30, L=30), roi_count=150),
    "count-over": lambda: _ptl(202, dict(F=40, B=200, M=30, L=30), roi_count=309),
    "count-0": lambda: _ptl(203, dict(F=40, B=200, M=30, L=30), roi_count=0),
    "mixed-fgover": lambda: _ptl(204, dict(F=40, B=200, M=30, L=30)),
    "mixed-fgunder": lambda: _ptl(205, dict(F=5, B=200, M=30, L=30)),
    "mixed-bgfew": lambda: _ptl(206, dict(F=40, B=10, M=30, L=30)),
    "fgonly-many": lambda: _ptl(207, dict(F=100, M=30, L=30)),
    "fgonly-5": lambda: _ptl(208, dict(F=5, M=30, L=30), rows=256, uniform5=True),
    "bgonly-many": lambda: _ptl(209, dict(B=100, M=30, L=30)),
    "bgonly-few": lambda: _ptl(210, dict(B=10, M=30, L=30)),
    "neither-mid": lambda: _ptl(211, dict(M=90)),
    "neither-low": lambda: _ptl(212, dict(L=90)),
    "equal": lambda: _ptl(213, {"=0.75": 6, "=0.5": 7, "=0.25": 8, "F": 3, "B": 9, "M": 5, "L": 5}),
    "skip-some": lambda: _ptl(214, dict(F=60, B=200, M=30, L=30), skip="some"),
    "skip-allfg": lambda: _ptl(215, {"F": 30, "=0.75": 4, "B": 200, "M": 30}, skip="allfg"),
    "nc2": lambda: _ptl(216, dict(F=40, B=200, M=30, L=30), num_classes=2),
    "noscores": lambda: _ptl(217, dict(F=40, B=200, M=30, L=30), scores=False),
    "gtcount-live": lambda: _ptl(218, dict(F=40, B=200, M=30, L=60), dead=3, gt_count=4),
    "gtcount-over": lambda: _ptl(218, dict(F=40, B=200, M=30, L=60), dead=3, gt_count=8),
    "gtcount-0": lambda: _ptl(218, dict(F=40, B=200, M=30, L=60), dead=3, gt_count=0),
})
PTL_CASES = [(c, e) for c in PTL_BUILDERS for e in (4, 7)]


def _ptl_id(case):
    return "%s-E%d" % case


def ptl_reference(inp, e):
    """Overlaps, first-maximum assignment, candidate sets, quotas and every row's normalised targets in float64
    (proposal_target_layer.py:194-231, :142-163)."""
    rois, gt = inp["rois"].astype(f64), inp["gt"].astype(f64)
    g = len(gt) if inp["gt_count"] is None else max(1, min(len(gt), inp["gt_count"]))
    r = len(rois)
    live = np.arange(r) < (r if inp["roi_count"] is None else min(inp["roi_count"], r))
    if inp["skip"] is not None:
        live &= inp["skip"] == 0
    ov = iou64(rois[:, 1:5], gt[:g, :4])
    assign, mx = ov.argmax(1), ov.max(1)
    fg_t, bg_hi, bg_lo = inp["th"]
    fg_c = live & (mx >= fg_t)
    bg_c = live & ~fg_c & (mx < bg_hi) & (mx >= bg_lo)
    nfg_c, nbg_c, rows = int(fg_c.sum()), int(bg_c.sum()), inp["rows"]
    quota = int(round(inp["frac"] * rows))
    if nfg_c and nbg_c:
        n_fg = min(quota, nfg_c)
        n_bg = rows - n_fg
    elif nfg_c:
        n_fg, n_bg = rows, 0
    else:
        n_fg, n_bg = 0, (rows if nbg_c else 0)
    if e == 7:
        t = encode_lidar64(rois[:, 1:5], inp["anchors_3d"], inp["true_gt"].astype(f64)[assign, :7])
    else:
        t = encode64(rois[:, 1:5], gt[assign, :4])
    means, stds = np.asarray(PTL_MEANS[:e], f32).astype(f64), np.asarray(PTL_STDS[:e], f32).astype(f64)   # what the kernel is given
    return dict(g=g, live=live, ov=ov, assign=assign.astype(np.int32), fg_c=fg_c, bg_c=bg_c, n_fg=n_fg, n_bg=n_bg,
                counts=[n_fg, n_bg, nfg_c, nbg_c], t=(t - means) / stds, cls=gt[assign, 4].astype(f32))


@functools.lru_cache(maxsize=None)
def ptl_case(case):
    cid, e = case
    inp = PTL_BUILDERS[cid]()
    ref = ptl_reference(inp, e)
    n_equal = _assert_clear(_ptl_id(case), ref["ov"].max(1), inp["th"])
    assert n_equal == (21 if cid == "equal" else 4 if cid == "skip-allfg" else 0), (case, n_equal)
    _assert_no_near_ties(_ptl_id(case), ref["ov"], 1)
    return inp, ref, dict(targets=PTL_BAR * _big(ref["t"]))


def ptl_check(case, out, side, headroom=1.0):
    """The invariants of one call's outputs (numpy).  ``assign`` / ``counts`` may be missing (the oracle returns neither)."""
    inp, ref, bars = ptl_case(case)
    cid, e = _ptl_id(case), case[1]
    rows, k = inp["rows"], inp["num_classes"]
    n_fg, n_bg = ref["n_fg"], ref["n_bg"]
    if out.get("counts") is not None:
        assert list(out["counts"]) == ref["counts"], (cid, side, list(out["counts"]), ref["counts"])
    assert out["rois"].shape == (rows, 5) and out["targets"].shape == (rows, e * k), (cid, side)
    j = np.arange(rows)
    used, is_fg = j < n_fg + n_bg, j < n_fg
    for name in ("rois", "labels", "scores", "targets", "inside", "outside", "assign", "anchors_3d"):
        if out.get(name) is not None:                             # rows nothing was drawn for: exactly zero
            assert not out[name][~used].any(), (cid, side, name, "an unused row is not zero")
    src = out["rois"][used, 0].astype(np.int64)
    assert ((src >= 0) & (src < len(inp["rois"]))).all(), (cid, side)
    _assert_bits("ptl", cid, "rois (%s)" % side, out["rois"][used], inp["rois"][src])
    assert ref["fg_c"][src[is_fg[used]]].all(), (cid, side, "a foreground row is no live unskipped fg candidate")
    assert ref["bg_c"][src[~is_fg[used]]].all(), (cid, side, "a background row is no live unskipped bg candidate")
    fg_src, bg_src = src[is_fg[used]], src[~is_fg[used]]
    if n_fg <= ref["counts"][2]:
        assert len(set(fg_src.tolist())) == n_fg, (cid, side, "fg rows repeat without need")
    if n_bg <= ref["counts"][3]:
        assert len(set(bg_src.tolist())) == n_bg, (cid, side, "bg rows repeat without need")
    want_scores = inp["scores"][src] if inp["scores"] is not None else np.zeros(len(src), f32)
    _assert_bits("ptl", cid, "scores (%s)" % side, out["scores"][used], want_scores)
    if out.get("assign") is not None:
        _assert_bits("ptl", cid, "assign (%s)" % side, out["assign"][used], ref["assign"][src])
    if e == 7:
        _assert_bits("ptl", cid, "anchors_3d (%s)" % side, out["anchors_3d"][used], inp["anchors_3d"][src])
    labels = np.zeros(rows, f32)
    labels[:n_fg] = ref["cls"][fg_src]
    _assert_bits("ptl", cid, "labels (%s)" % side, out["labels"], labels)
    want_t, want_w = np.zeros((rows, e * k)), np.zeros((rows, e * k), f32)
    for row in np.flatnonzero(labels > 0):
        c = int(labels[row])
        want_t[row, e * c:e * c + e] = ref["t"][src[row]]
        want_w[row, e * c:e * c + e] = 1
    _assert_close("ptl", cid, "targets", out["targets"], want_t, bars["targets"], side, headroom)
    assert not out["targets"][want_w == 0].any(), (cid, side, "targets outside the assigned class's columns")
    _assert_bits("ptl", cid, "inside (%s)" % side, out["inside"], want_w)
    _assert_bits("ptl", cid, "outside (%s)" % side, out["outside"], want_w)
    if inp["uniform5"]:
        # 256 rows drawn with replacement from 5 candidates: a candidate's count is Binomial(256, 1/5), mean 51.2,
        # sigma = sqrt(256 * 0.2 * 0.8) = 6.4, 6 sigma = 38.4; P(|z| > 6) = 2e-9 per candidate
        assert n_fg == 256 and ref["counts"][2] == 5
        ok, dev = _within_sigmas(np.bincount(fg_src, minlength=len(inp["rois"]))[ref["fg_c"]], 256, 0.2)
        assert ok, "%s (%s): a candidate's count is %.2f sigma from 51.2" % (cid, side, dev)


def _ptl_oracle(inp, ref, e, seed):
    """oracle.proposal_target_layer on the live, unskipped rows and the live gt rows (it has no roi_count / skip_mask /
    gt_count); the row id in column 0 still names the source row."""
    sel = np.flatnonzero(ref["live"])
    scores = inp["scores"] if inp["scores"] is not None else np.zeros(len(inp["rois"]), f32)
    fg_t, bg_hi, bg_lo = inp["th"]
    with _oracle_settings(TRAIN_ROI_BATCH_SIZE=inp["rows"], TRAIN_FG_FRACTION=inp["frac"], TRAIN_FG_THRESH=fg_t, TRAIN_BG_THRESH_HI=bg_hi,
                          TRAIN_BG_THRESH_LO=bg_lo, BBOX_NORMALIZE_MEANS=PTL_MEANS[:4], BBOX_NORMALIZE_STDS=PTL_STDS[:4],
                          LIDAR_BBOX_NORMALIZE_MEANS=PTL_MEANS, LIDAR_BBOX_NORMALIZE_STDS=PTL_STDS):
        lab, rois, a3, sc, tgt, inw, outw = O.proposal_target_layer(
            torch.from_numpy(inp["rois"][sel]), torch.from_numpy(scores[sel]).view(-1, 1), torch.from_numpy(inp["anchors_3d"][sel]),
            torch.from_numpy(inp["gt"][:ref["g"]]), torch.from_numpy(inp["true_gt"][:ref["g"]]), inp["num_classes"], e,
            net_type="lidar" if e == 7 else "image", generator=torch.Generator().manual_seed(seed))
    return dict(labels=_np(lab).reshape(-1), rois=_np(rois), scores=_np(sc), anchors_3d=_np(a3) if e == 7 else None, targets=_np(tgt),
                inside=_np(inw), outside=_np(outw))


@pytest.mark.parametrize("case", PTL_CASES, ids=_ptl_id)
def test_cpu_restatement_proposal_target_layer(case):
    inp, ref, bars = ptl_case(case)
    cid, e = _ptl_id(case), case[1]
    # float32 classifies like float64: the kernel's IoU, first maximum, and the three comparisons
    ov = iou32(inp["rois"][:, 1:5], inp["gt"][:ref["g"], :4])
    assert np.array_equal(ov, _np(O.bbox_overlaps(inp["rois"][:, 1:5], inp["gt"][:ref["g"], :4]))), cid
    mx = ov.max(1)
    fg_t, bg_hi, bg_lo = (f32(v) for v in inp["th"])
    assert np.array_equal(ov.argmax(1), ref["assign"]), cid
    fg_c = ref["live"] & (mx >= fg_t)
    assert np.array_equal(fg_c, ref["fg_c"]) and np.array_equal(ref["live"] & ~fg_c & (mx < bg_hi) & (mx >= bg_lo), ref["bg_c"]), cid
    assert int(np.rint(f32(inp["frac"]) * f32(inp["rows"]))) == int(round(inp["frac"] * inp["rows"]))       # lrintf
    # every row's normalised targets, float32 in the kernel's order
    gt = inp["gt"]
    if e == 7:
        t32 = encode_lidar32(inp["rois"][:, 1:5], inp["anchors_3d"], inp["true_gt"][ref["assign"], :7])
        t_or = O.lidar_3d_bbox_transform(torch.from_numpy(inp["rois"][:, 1:5]).double(), torch.from_numpy(inp["anchors_3d"]).double(),
                                         torch.from_numpy(inp["true_gt"][ref["assign"], :7]).double())
    else:
        t32 = encode32(inp["rois"][:, 1:5], gt[ref["assign"], :4])
        t_or = O.bbox_transform(torch.from_numpy(inp["rois"][:, 1:5]).double(), torch.from_numpy(gt[ref["assign"], :4]).double())
    means, stds = np.asarray(PTL_MEANS[:e], f32), np.asarray(PTL_STDS[:e], f32)
    _assert_close("ptl", cid, "targets of every row", (t32 - means) / stds, ref["t"], bars["targets"], "restated", HEADROOM)
    _assert_close("ptl", cid, "targets of every row", (_np(t_or) - means.astype(f64)) / stds.astype(f64), ref["t"],
                  1e-12 * _big(ref["t"]), "oracle float64")
    if ref["n_fg"] + ref["n_bg"] == 0:
        if ref["live"].any():
            with pytest.raises(RuntimeError, match="no foreground and no background"):
                _ptl_oracle(inp, ref, e, 3)                       # the reference stops in a debugger here
        assert ref["counts"] == [0, 0, 0, 0]
    else:
        ptl_check(case, _ptl_oracle(inp, ref, e, 3), "oracle")   # the reference's own draw passes the device's checks
    if inp["gt_count"] is not None and inp["gt_count"] < len(gt):  # the dead rows matter: read, the far rows become fg
        assert ptl_reference(dict(inp, gt_count=None), e)["counts"] != ref["counts"], cid
    if case[0] == "skip-allfg":
        assert ref["counts"][:3] == [0, inp["rows"], 0] and ptl_reference(dict(inp, skip=None), e)["counts"][2] == 34
    if case[0] in ("mixed-fgover", "nc2", "fgonly-many"):          # a class-0 box among the fg candidates' boxes, and a tie with row 3
        assert (ref["cls"][ref["fg_c"]] == 0).any() and (ref["ov"][ref["fg_c"], 0] == ref["ov"][ref["fg_c"], 3]).any(), cid
    if case[0] == "equal":
        assert ref["counts"][2:] == [9, 17]                       # 6 at 0.75 + 3 F; 8 at 0.25 + 9 B; the 7 at 0.5 are neither


def _ptl_run(inp, e, seed, seed_dev=None, gt_count="case"):
    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

    cnt = inp["gt_count"] if gt_count == "case" else gt_count
    sd = None if seed_dev is None else torch.tensor([seed_dev - (1 << 32) if seed_dev >= (1 << 31) else seed_dev], dtype=torch.int32,
                                                    device=DEV)
    fg_t, bg_hi, bg_lo = inp["th"]
    out = _ops().proposal_target_layer(
        dev(inp["rois"]), dev(inp["scores"]), dev(inp["gt"]), inp["num_classes"], inp["rows"], inp["frac"], fg_t, bg_hi, bg_lo,
        PTL_MEANS[:e], PTL_STDS[:e], seed,
        roi_count=None if inp["roi_count"] is None else torch.tensor([inp["roi_count"]], dtype=torch.int32, device=DEV),
        anchors_3d=dev(inp["anchors_3d"]) if e == 7 else None, true_gt_boxes=dev(inp["true_gt"]) if e == 7 else None,
        skip_mask=dev(inp["skip"]), seed_dev=sd,
        gt_count=None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device=DEV))
    return {k: _np(v) for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", PTL_CASES, ids=_ptl_id)
def test_proposal_target_layer(hip, case):
    inp, ref, _ = ptl_case(case)
    e = case[1]
    out = _ptl_run(inp, e, 11)
    ptl_check(case, out, "device")
    if ref["n_fg"] + ref["n_bg"] == 0:                           # pinned: where the reference stops, all-zero rows and counts
        assert list(out["counts"]) == [0, 0, 0, 0] and not any(v.any() for v in out.values())
    if inp["gt_count"] is not None:                              # bit for bit the call on the clamped number of rows
        rows = ref["g"]
        _same_bits("ptl", _ptl_id(case), "gt_count vs %d rows" % rows, out,
                   _ptl_run(dict(inp, gt=inp["gt"][:rows].copy(), true_gt=inp["true_gt"][:rows].copy()), e, 11, gt_count=None))


@pytest.mark.parametrize("e", (4, 7))
def test_cpu_restatement_proposal_target_layer_rejects_4097(e):
    """ptl_kernel is one workgroup with its keys in LDS: 4096 RoIs take 2 * 4096 * 8 + 4096 * 4 = 80 KB of the 160 KB; the
    entry point refuses more rather than sample from a prefix."""
    assert 2 * 4096 * 8 + 4096 * 4 == 80 * 1024
    assert len(ptl_case(("R4096", e))[0]["rois"]) == 4096


@pytest.mark.gpu
@pytest.mark.parametrize("e", (4, 7))
def test_proposal_target_layer_rejects_4097(hip, e):
    from faster_rcnn_pytorch_multimodal_amd import _hip
    inp = dict(ptl_case(("R4096", e))[0])
    inp["rois"] = np.concatenate((inp["rois"], inp["rois"][:1]))
    inp["scores"] = np.concatenate((inp["scores"], inp["scores"][:1]))
    inp["anchors_3d"] = np.concatenate((inp["anchors_3d"], inp["anchors_3d"][:1]))
    with pytest.raises(_hip.HipError, match="num_rois <= 4096"):
        _ptl_run(inp, e, 1)


@pytest.mark.parametrize("e", (4, 7))
@pytest.mark.parametrize("pair", list(SEED_PAIRS))
def test_cpu_restatement_proposal_target_layer_seeds(pair, e):
    """The case leaves the draw a choice (16 of 40 fg, 48 of 200 bg), so two draws agree by chance with probability below
    1e-10; the reference's two draws differ."""
    s, d = SEED_PAIRS[pair]
    assert ((s + d) >= 2 ** 32) == (pair != "small")
    inp, ref, _ = ptl_case(("mixed-fgover", e))
    assert ref["counts"] == [16, 48, 40, 200]
    assert not np.array_equal(_ptl_oracle(inp, ref, e, 1)["rois"], _ptl_oracle(inp, ref, e, 2)["rois"])


@pytest.mark.gpu
@pytest.mark.parametrize("e", (4, 7))
@pytest.mark.parametrize("pair", list(SEED_PAIRS))
def test_proposal_target_layer_seeds(hip, pair, e):
    inp, _, _ = ptl_case(("mixed-fgover", e))
    s, d = SEED_PAIRS[pair]
    total = (s + d) & 0xFFFFFFFF
    one = _ptl_run(inp, e, total)
    _same_bits("ptl", pair, "same seed", one, _ptl_run(inp, e, total))
    _same_bits("ptl", pair, "seed + seed_dev", one, _ptl_run(inp, e, s, seed_dev=d))
    assert not np.array_equal(one["rois"], _ptl_run(inp, e, (total + 1) & 0xFFFFFFFF)["rois"])
    ptl_check(("mixed-fgover", e), one, "device")
