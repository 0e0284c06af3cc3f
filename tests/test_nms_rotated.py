"""Rotated BEV NMS (cfg.TEST.NMS_ROTATED): ``utils.bbox.nms_rotated_host``, ``ops.nms_rotated``,
``ops.filter_per_class_lidar(rotated=True)`` and the switch's way through ``filter_device`` and the captured frame.

The yardstick is always ``waymo_eval.iou(bbgt=box_i[None], bb=box_j, 'bev')`` for i < j in (score descending, index
ascending) order plus the greedy loop of THIS file (``greedy``) - never the device code and never ``nms_rotated_host``,
which is itself under test.

Exactness.  The device restates ``iou`` term for term in float64; what differs is its cos / sin and numpy's BLAS dot in
the shoelace sum, 1.2e-12 at the most on an MI355X (profiles/device_eval.md).  Every scene is therefore checked, from the
HOST overlaps alone, to hold no pair within ``MARGIN`` = 1e-6 of the threshold (the seeded scenes of ``ops.nms_rotated``
in both argument orders); kept sets are then compared exactly.  The seeds were chosen on the CPU so that this holds.

Host overlaps cost about 46 us a pair: one 200-box scene is shared by every size (its prefixes) and threshold, the filter
scenes are cached per size.
"""
import functools

import numpy as np
import pytest

from faster_rcnn_pytorch_multimodal_amd.datasets.waymo_eval import iou
from faster_rcnn_pytorch_multimodal_amd.model import config as C
from faster_rcnn_pytorch_multimodal_amd.utils.bbox import nms_rotated_host

MARGIN = 1e-6
DEV = "cuda:0"
SCENE_SEED, SCENE_N = 0, 200
SIZES = (1, 2, 63, 64, 65, 129, 200)
THRESHOLDS = (0.1, 0.3, 0.6)


# ---- the host yardstick -----------------------------------------------------------------------------------------------
def dense_scene(n, seed):
    """n boxes of 3 to 5.5 m x 1.5 to 2.4 m with uniform yaw on a 30 x 20 m patch, float32 [xc,yc,zc,l,w,h,ry]."""
    rng = np.random.default_rng(seed)
    cols = (rng.uniform(0, 30, n), rng.uniform(0, 20, n), rng.uniform(-1, 1, n), rng.uniform(3, 5.5, n),
            rng.uniform(1.5, 2.4, n), rng.uniform(1.4, 2.0, n), rng.uniform(-np.pi, np.pi, n))
    return np.stack(cols, 1).astype(np.float32)


def host_overlaps(boxes, both=False):
    """ov[i, j] = iou(bbgt=box_i[None], bb=box_j, 'bev') for i < j (NaN elsewhere); with ``both`` also the other argument
    order rev[i, j] = iou(bbgt=box_j[None], bb=box_i)."""
    b = np.asarray(boxes, dtype=np.float64)
    n = b.shape[0]
    ov = np.full((n, n), np.nan)
    rev = np.full((n, n), np.nan) if both else None
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(1, n):
            ov[:j, j] = iou(b[:j], b[j], "bev")
        if both:
            for i in range(n - 1):
                rev[i, i + 1:] = iou(b[i + 1:], b[i], "bev")
    return (ov, rev) if both else ov


def greedy(ov, n, thresh, at_equal=True):
    """Kept positions among the first n boxes of the order ``ov`` was computed in; thresh is the float32 the device gets."""
    t = float(np.float32(thresh))
    kept = []
    for j in range(n):
        pre = ov[kept, j]                                 # NaN compares false: never suppresses
        if kept and (np.any(pre >= t) if at_equal else np.any(pre > t)):
            continue
        kept.append(j)
    return kept


def margin_of(ov, n, thresh):
    """Smallest |overlap - thresh| over the pairs i < j < n (NaN overlaps cannot be near anything)."""
    d = np.abs(ov[:n, :n] - float(np.float32(thresh)))
    return np.nanmin(d) if np.isfinite(d).any() else np.inf


@functools.lru_cache(maxsize=None)
def shared_scene():
    boxes = dense_scene(SCENE_N, SCENE_SEED)
    ov, rev = host_overlaps(boxes, both=True)
    for a in (boxes, ov, rev):
        a.setflags(write=False)
    return boxes, ov, rev


PI = float(np.pi)
PERPENDICULAR = np.array([[0, 0, 0, 4.5, 1.8, 1.5, 0], [0, 0, 0, 4.5, 1.8, 1.5, PI / 2]], np.float32)
SAME_CAR = np.array([[0, 0, 0, 4.5, 1.8, 1.5, 0], [0, 0, 0, 1.8, 4.5, 1.5, PI / 2]], np.float32)
TIE = np.array([[0, 0, 0, 4, 2, 1.5, 0], [1, 0, 0, 2, 2, 1.5, 0]], np.float32)
# (boxes, thresh, at_equal, kept positions)
HAND_CASES = [(PERPENDICULAR, 0.6, True, [0, 1]), (SAME_CAR, 0.6, True, [0]), (TIE, 0.5, True, [0]), (TIE, 0.5, False, [0, 1])]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_switch_is_off_by_default():
    C.reset_cfg()
    assert C.cfg.TEST.NMS_ROTATED is False


@pytest.mark.parametrize("case", range(len(HAND_CASES)))
def test_host_rule_on_hand_built_cases(case):
    boxes, thresh, at_equal, want = HAND_CASES[case]
    ov = host_overlaps(boxes)
    assert greedy(ov, len(boxes), thresh, at_equal) == want         # the yardstick says what the issue's table says
    scores = np.array([0.9, 0.8], np.float32)
    assert nms_rotated_host(boxes, scores, thresh, at_equal=at_equal).tolist() == want
    # scores pick the order: the other box first, the kept indices are indices into the INPUT
    flipped = nms_rotated_host(boxes[::-1], scores[::-1], thresh, at_equal=at_equal).tolist()
    assert flipped == [1 - k for k in greedy(host_overlaps(boxes), len(boxes), thresh, at_equal)]


def test_host_tie_is_exact_in_both_argument_orders():
    assert iou(TIE[:1], TIE[1], "bev")[0] == 0.5 and iou(TIE[1:], TIE[0], "bev")[0] == 0.5


def test_host_rule_on_a_dense_scene_and_its_refusals():
    boxes, ov, _ = shared_scene()
    n = 64
    rng = np.random.default_rng(5)
    scores = np.round(rng.uniform(0.1, 1.0, n) * 16) / 16           # ties: broken by index
    order = np.lexsort((np.arange(n), -scores))
    ov_sorted = host_overlaps(boxes[:n][order])
    for thresh in (0.6, 0.1):
        want = [int(order[k]) for k in greedy(ov_sorted, n, thresh)]
        assert nms_rotated_host(boxes[:n], scores, thresh).tolist() == want
    assert len(want) < n                                             # at 0.1 something is suppressed
    for bad in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="must be > 0"):
            nms_rotated_host(boxes[:4], scores[:4], bad)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _dev_nms(boxes, thresh, n_dev=None, max_keep=None):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    b = torch.from_numpy(np.array(boxes, dtype=np.float32)).to(DEV)
    cnt = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    keep_idx, keep_count = ops.nms_rotated(b, thresh, n=cnt, max_keep=max_keep)
    torch.cuda.synchronize()
    return keep_idx.cpu().numpy(), int(keep_count.item())


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_device_nms_on_seeded_dense_scenes(hip, n, thresh):
    boxes, ov, rev = shared_scene()
    m, m_rev = margin_of(ov, n, thresh), margin_of(rev, n, thresh)
    print("n %d thresh %.1f: margin %.3e (other argument order %.3e)" % (n, thresh, m, m_rev))
    assert m > MARGIN and m_rev > MARGIN, "the scene holds a pair within 1e-6 of the threshold: pick another seed"
    want = greedy(ov, n, thresh)
    keep_idx, count = _dev_nms(boxes[:n], thresh)
    assert count == len(want)
    assert keep_idx[:count].tolist() == want
    assert not keep_idx[count:].any()                                  # the unused tail is written as 0


@pytest.mark.gpu
def test_scene_discriminates_rotated_from_yaw_less(hip):
    """On the 200-box scene at 0.6 the yaw-less rule (ops.nms_sorted on xc -+ l/2, yc -+ w/2) keeps another set."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    boxes, ov, _ = shared_scene()
    rect = np.stack((boxes[:, 0] - boxes[:, 3] / 2, boxes[:, 1] - boxes[:, 4] / 2, boxes[:, 0] + boxes[:, 3] / 2,
                     boxes[:, 1] + boxes[:, 4] / 2), 1).astype(np.float32)
    idx, cnt, _ = ops.nms_sorted(torch.from_numpy(rect).to(DEV), 0.6)
    yaw_less = idx.cpu().numpy()[:int(cnt.item())].tolist()
    rotated = _dev_nms(boxes, 0.6)
    assert rotated[0][:rotated[1]].tolist() == greedy(ov, SCENE_N, 0.6)
    assert yaw_less != greedy(ov, SCENE_N, 0.6)


@pytest.mark.gpu
@pytest.mark.parametrize("n_max,n_dev", [(129, 100), (200, 65), (64, 0)])
def test_device_nms_reads_the_live_count_on_the_device(hip, n_max, n_dev):
    boxes, ov, _ = shared_scene()
    assert margin_of(ov, n_dev, 0.3) > MARGIN
    want = greedy(ov, n_dev, 0.3)
    keep_idx, count = _dev_nms(boxes[:n_max], 0.3, n_dev=n_dev)
    assert count == len(want) and keep_idx[:count].tolist() == want and not keep_idx[count:].any()


@pytest.mark.gpu
def test_device_nms_max_keep_cuts_the_kept_list(hip):
    boxes, ov, _ = shared_scene()
    want = greedy(ov, 129, 0.3)
    assert len(want) > 10
    keep_idx, count = _dev_nms(boxes[:129], 0.3, max_keep=10)
    assert keep_idx.shape == (10,) and count == 10 and keep_idx.tolist() == want[:10]


@pytest.mark.gpu
def test_device_nms_hand_built_cases_and_the_tie_rule(hip):
    from faster_rcnn_pytorch_multimodal_amd import ops
    old = ops.nms_suppress_at_equal()
    try:
        for boxes, thresh, at_equal, want in HAND_CASES:
            ops.set_nms_suppress_at_equal(at_equal)
            assert greedy(host_overlaps(boxes), len(boxes), thresh, at_equal) == want
            keep_idx, count = _dev_nms(boxes, thresh)
            assert keep_idx[:count].tolist() == want, (boxes, thresh, at_equal)
    finally:
        ops.set_nms_suppress_at_equal(old)


def degenerate_scene():
    """40 scene boxes with degenerate copies of scene boxes mixed in (each copy sits on the box it was made from, so it
    overlaps it and its neighbours, both as a predecessor and as a successor): a NaN in each of the seven fields in turn,
    l = 0, w = 0, a negative w, ry = 1e6.  The host functions raise for none of them and every answer is plain IEEE
    arithmetic (a NaN or zero-area overlap compares false; a negative w gives a clockwise rectangle whose clip is empty
    or whose union is negative), so no row is left out."""
    base = dense_scene(40, 3)
    rows, src = [], 0
    edits = [(k, np.nan) for k in range(7)] + [(3, 0.0), (4, 0.0), (4, -2.0), (6, 1e6)]
    out = []
    for pos in range(len(base)):
        out.append(base[pos])
        if pos % 3 == 1 and src < len(edits):
            r = base[pos + 1 if src % 2 else pos].copy()             # a copy of the next box or of this one
            r[edits[src][0]] = edits[src][1]
            out.append(r)
            rows.append(len(out) - 1)
            src += 1
    assert src == len(edits)
    return np.stack(out).astype(np.float32), rows


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", (0.1, 0.6))
def test_device_nms_degenerate_rows(hip, thresh):
    """NaN fields, zero and negative extents and ry = 1e6 mixed into a scene: the keep set equals the host rule's and the
    call returns FRCNN_OK (ops raises otherwise).  All eleven kinds of row stay in (see ``degenerate_scene``)."""
    boxes, rows = degenerate_scene()
    assert len(rows) == 11 and np.isnan(boxes[rows[:7]]).sum() == 7
    ov = host_overlaps(boxes)
    assert margin_of(ov, len(boxes), thresh) > MARGIN
    want = greedy(ov, len(boxes), thresh)
    assert set(rows) & set(want) and len(want) < len(boxes)
    keep_idx, count = _dev_nms(boxes, thresh)
    assert keep_idx[:count].tolist() == want


# ---- the per-class filter -----------------------------------------------------------------------------------------------
K_FILTER = 3
FILTER_SEEDS = {1: 1, 65: 1, 300: 1}
ROI_COUNTS = {1: 1, 65: 60, 300: 281}
SCORE_THRESH, NMS_THRESH = 0.1, 0.6


def detector_scene(n, seed):
    """What a detector hands the filter: ceil(n / 3) cars on the 30 x 20 m patch, each predicted about three times with
    jitter (centre 0.15 m, extents 3 %, yaw 0.05 rad), a third of the predictions in the other anchor's form
    (l and w swapped, ry + pi/2) - the same footprint, which only the rotated rule recognises."""
    rng = np.random.default_rng(seed)
    cars = dense_scene((n + 2) // 3, seed + 7)
    rows = cars[rng.integers(0, len(cars), n)].astype(np.float64)
    rows[:, 0:2] += rng.normal(0, 0.15, (n, 2))
    rows[:, 3:6] *= 1 + rng.normal(0, 0.03, (n, 3))
    rows[:, 6] += rng.normal(0, 0.05, n)
    swap = rng.random(n) < 1 / 3
    rows[swap, 3], rows[swap, 4] = rows[swap, 4], rows[swap, 3]
    rows[swap, 6] += np.pi / 2
    return rows.astype(np.float32)


def filter_inputs(R, seed):
    """pred_boxes (R, 7K), cls_prob (R, K): a detector scene per class, scores on a grid of 1/32 (ties within and across
    the max_dets cut), about a third of them below the score threshold."""
    rng = np.random.default_rng(seed)
    pb = np.concatenate([detector_scene(R, 1000 * seed + c) for c in range(K_FILTER)], 1)
    cp = (np.round(rng.uniform(0.0, 1.0, (R, K_FILTER)) ** 2 * 32) / 32).astype(np.float32)
    return np.ascontiguousarray(pb, dtype=np.float32), np.ascontiguousarray(cp)


def host_kept(pb, cp, roi_count, thresh, nms_thresh, at_equal=True):
    """Per class: threshold, sort by (score descending, index ascending), rotated greedy.  Returns per class (kept RoI
    indices, the margin of the class's overlaps)."""
    res = [([], np.inf)]
    for c in range(1, cp.shape[1]):
        s = cp[:roi_count, c]
        inds = np.where(s > np.float32(thresh))[0]
        order = inds[np.lexsort((inds, -s[inds]))]
        ov = host_overlaps(pb[order, 7 * c:7 * c + 7])
        kept = [int(order[k]) for k in greedy(ov, len(order), nms_thresh, at_equal)]
        res.append((kept, margin_of(ov, len(order), nms_thresh)))
    return res


def host_filter(pb, cp, roi_count, thresh, nms_thresh, max_dets, kept=None):
    """``host_kept`` and the max_dets rule of lib/model/test.py:213-221 (ties with the max_dets-th score stay).  Returns
    per class (kept RoI indices before the cut, after the cut, the margin)."""
    kept = host_kept(pb, cp, roi_count, thresh, nms_thresh) if kept is None else kept
    res = []
    for c, (k, margin) in enumerate(kept):
        cut = k
        if max_dets > 0 and len(k) > max_dets:
            bound = np.sort(cp[k, c])[-max_dets]
            cut = [r for r in k if cp[r, c] >= bound]
        res.append((k, cut, margin))
    return res


@functools.lru_cache(maxsize=None)
def filter_case(R):
    """Inputs, a max_dets that cuts through a score tie of class 1, and the host reference."""
    pb, cp = filter_inputs(R, FILTER_SEEDS[R])
    kept = host_kept(pb, cp, ROI_COUNTS[R], SCORE_THRESH, NMS_THRESH)
    kept1 = kept[1][0]
    ties = [m for m in range(3, len(kept1)) if cp[kept1[m - 1], 1] == cp[kept1[m], 1]]   # kept scores descend
    max_dets = 1 if R == 1 else (ties[0] if ties else 0)
    return pb, cp, max_dets, host_filter(pb, cp, ROI_COUNTS[R], SCORE_THRESH, NMS_THRESH, max_dets, kept=kept)


def _run_filter(pb, cp, roi_count, max_dets, want_rois, **kw):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    pbd, cpd = torch.from_numpy(pb).to(DEV), torch.from_numpy(cp).to(DEV)
    cnt = torch.tensor([roi_count], dtype=torch.int32, device=DEV)
    out = ops.filter_per_class_lidar(pbd, cpd, SCORE_THRESH, NMS_THRESH, max_dets, None, roi_count=cnt,
                                     want_rois=want_rois, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _run_filter_poisoned(lib, pb, cp, roi_count, max_dets, want_rois):
    """frcnn_filter_per_class_lidar_rot through the C ABI into outputs pre-filled with a poison value: what comes back
    clean was written by the call."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip
    R, K = cp.shape
    pbd, cpd = torch.from_numpy(pb).to(DEV), torch.from_numpy(cp).to(DEV)
    cnt = torch.tensor([roi_count], dtype=torch.int32, device=DEV)
    dets = torch.full((K, R, 8), float("nan"), dtype=torch.float32, device=DEV)
    det_count = torch.full((K,), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    det_roi = torch.full((K, R), 0x7F7F7F7F, dtype=torch.int32, device=DEV) if want_rois else None
    ws_bytes = lib.frcnn_filter_per_class_lidar_rot_ws_bytes(R, K)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=DEV)
    _hip.check(lib.frcnn_filter_per_class_lidar_rot(pbd.data_ptr(), cpd.data_ptr(), cnt.data_ptr(), R, K, SCORE_THRESH,
                                                    NMS_THRESH, max_dets, R, dets.data_ptr(), det_count.data_ptr(),
                                                    None if det_roi is None else det_roi.data_ptr(), ws.data_ptr(), ws_bytes,
                                                    torch.cuda.current_stream().cuda_stream),
               "frcnn_filter_per_class_lidar_rot")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (dets, det_count, det_roi) if t is not None]


@pytest.mark.gpu
@pytest.mark.parametrize("want_rois", (False, True))
@pytest.mark.parametrize("R", (1, 65, 300))
def test_filter_rotated_against_the_host_reference(hip, R, want_rois):
    pb, cp, max_dets, ref = filter_case(R)
    for c in range(1, K_FILTER):
        print("R %d class %d: %d kept, %d after max_dets %d, margin %.3e" % (R, c, len(ref[c][0]), len(ref[c][1]), max_dets,
                                                                             ref[c][2]))
        assert ref[c][2] > MARGIN, "a pair within 1e-6 of the threshold: pick another seed"
    if R > 1:
        kept, cut, _ = ref[1]
        assert len(kept) > len(cut) > max_dets > 0, "max_dets must cut through a score tie and still drop something"
        assert len(kept) < (cp[:ROI_COUNTS[R], 1] > SCORE_THRESH).sum()   # the rotated rule suppressed something
    out = _run_filter_poisoned(hip, pb, cp, ROI_COUNTS[R], max_dets, want_rois)
    through_ops = _run_filter(pb, cp, ROI_COUNTS[R], max_dets, want_rois, rotated=True)
    assert len(out) == len(through_ops) == (3 if want_rois else 2)
    for a, b in zip(out, through_ops):
        assert a.tobytes() == b.tobytes()
    dets, det_count = out[0], out[1]
    assert dets.shape == (K_FILTER, R, 8) and det_count.shape == (K_FILTER,)
    want_dets = np.zeros((K_FILTER, R, 8), np.float32)
    want_roi = np.full((K_FILTER, R), -1, np.int32)
    for c in range(1, K_FILTER):
        cut = ref[c][1]
        want_dets[c, :len(cut), :7] = pb[cut, 7 * c:7 * c + 7]
        want_dets[c, :len(cut), 7] = cp[cut, c]
        want_roi[c, :len(cut)] = cut
    np.testing.assert_array_equal(det_count, [0] + [len(ref[c][1]) for c in range(1, K_FILTER)])
    np.testing.assert_array_equal(dets, want_dets)                    # rows beyond the count are zero, class 0 is empty
    if want_rois:
        np.testing.assert_array_equal(out[2], want_roi)               # -1 beyond the count


@pytest.mark.gpu
def test_filter_rotated_empty_frame(hip):
    """roi_count 0 on the device: every class is empty, every element is still written."""
    pb, cp = filter_inputs(65, 2)
    dets, det_count, det_roi = _run_filter(pb, cp, 0, 5, True, rotated=True)
    assert not dets.any() and not det_count.any() and (det_roi == -1).all()


@pytest.mark.gpu
def test_filter_rotated_refusals(hip):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    pb, cp = filter_inputs(1025, 2)
    pbd, cpd = torch.from_numpy(pb).to(DEV), torch.from_numpy(cp).to(DEV)
    with pytest.raises(_hip.HipError, match="num_rois 1025 > 1024"):
        ops.filter_per_class_lidar(pbd, cpd, 0.1, 0.6, 0, rotated=True)
    with pytest.raises(_hip.HipError, match="must be > 0"):
        ops.filter_per_class_lidar(pbd[:65].contiguous(), cpd[:65].contiguous(), 0.1, 0.0, 0, rotated=True)
    with pytest.raises(_hip.HipError, match="must be > 0"):
        ops.nms_rotated(pbd[:65, :7].contiguous(), 0.0)
    with pytest.raises(_hip.HipError, match="n_max 4097 > 4096"):
        ops.nms_rotated(torch.zeros((4097, 7), device=DEV), 0.5)
    # a short workspace, through the C ABI
    lib = _hip.load()
    R, K = 65, K_FILTER
    need = lib.frcnn_filter_per_class_lidar_rot_ws_bytes(R, K)
    assert need > 0 and lib.frcnn_filter_per_class_lidar_rot_ws_bytes(1025, K) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dets = torch.empty((K, R, 8), device=DEV)
    cnt = torch.empty((K,), dtype=torch.int32, device=DEV)
    rc = lib.frcnn_filter_per_class_lidar_rot(pbd[:R].contiguous().data_ptr(), cpd[:R].contiguous().data_ptr(), None, R, K,
                                              0.1, 0.6, 0, R, dets.data_ptr(), cnt.data_ptr(), None, ws.data_ptr(), need - 1,
                                              None)
    with pytest.raises(_hip.HipError, match="workspace"):
        _hip.check(rc, "frcnn_filter_per_class_lidar_rot")
    need1 = lib.frcnn_nms_rotated_ws_bytes(R)
    rc = lib.frcnn_nms_rotated(pbd[:R, :7].contiguous().data_ptr(), None, R, 0.5, R, ws.data_ptr(), None, cnt.data_ptr(),
                               ws.data_ptr(), need1 - 1, None)
    with pytest.raises(_hip.HipError, match="workspace"):
        _hip.check(rc, "frcnn_nms_rotated")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_rotated_false_is_the_default_call_and_filter_device_follows_the_switch(hip):
    import torch
    from faster_rcnn_pytorch_multimodal_amd.utils.filter_predictions import filter_device
    pb, cp, _, ref = filter_case(65)
    max_dets = 0                                     # no cut: the two rules keep 29 and 21 boxes of class 1 here
    plain = _run_filter(pb, cp, ROI_COUNTS[65], max_dets, True)
    off = _run_filter(pb, cp, ROI_COUNTS[65], max_dets, True, rotated=False)
    on = _run_filter(pb, cp, ROI_COUNTS[65], max_dets, True, rotated=True)
    for a, b in zip(plain, off):
        assert a.tobytes() == b.tobytes()                             # bit-equal
    assert any(a.tobytes() != b.tobytes() for a, b in zip(plain, on)), "the scene does not tell the two rules apart"
    pbd, cpd = torch.from_numpy(pb).to(DEV), torch.from_numpy(cp).to(DEV)
    cnt = torch.tensor([ROI_COUNTS[65]], dtype=torch.int32, device=DEV)
    C.reset_cfg()
    try:
        assert C.cfg.TEST.NMS_THRESH == NMS_THRESH
        for switch, want in ((True, on), (False, plain)):
            C.cfg.TEST.NMS_ROTATED = switch
            dets, det_count = filter_device(cnt, cpd, pbd, None, SCORE_THRESH, max_dets, None, db_type="lidar")
            assert dets.cpu().numpy().tobytes() == want[0].tobytes() and det_count.cpu().numpy().tobytes() == want[1].tobytes()
            # the uncertainty columns ride on det_roi: a column holding each RoI's own index comes back as det_roi
            unc = {"a_entropy": torch.arange(65, dtype=torch.float32, device=DEV)}
            wide, _ = filter_device(cnt, cpd, pbd, None, SCORE_THRESH, max_dets, None, db_type="lidar", uncertainties=unc)
            wide = wide.cpu().numpy()
            assert wide.shape == (K_FILTER, 65, 9) and wide[:, :, :8].tobytes() == want[0].tobytes()
            np.testing.assert_array_equal(wide[:, :, 8], np.maximum(want[2], 0))
    finally:
        C.reset_cfg()


# ---- end to end: the captured frame ---------------------------------------------------------------------------------------
# Seeded weights spread the frame's 286 boxes thinly (largest rotated IoU 0.46): at cfg.TEST.NMS_THRESH = 0.2 the rotated
# rule keeps 202 of them and the yaw-less rule 175 (margin 3.5e-5, measured on an MI355X), so the frame tells them apart.
FRAME_SEED, FRAME_THRESH, FRAME_MAX_DETS, FRAME_NMS_THRESH = 9, 0.05, 0, 0.2


@pytest.mark.gpu
def test_captured_lidar_frame_follows_the_switch(hip):
    """The smallest LiDAR detector of the suite (2 classes, a 208 x 176 x 15 BEV blob, seeded weights) through the frame
    pool with cfg.TEST.FRAME_GRAPHS: with the switch on the replayed detections equal the eager ones bit for bit and the
    host reference applied to the frame's eager cls_prob / pred_boxes; a second frame of the same shape with the switch
    off has another frame-graph key and follows the yaw-less rule.  No max_dets cut here (the filter tests cover it)."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device
    from faster_rcnn_pytorch_multimodal_amd.nets.lidarnet import lidarnet
    from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
    C.reset_cfg()
    try:
        C.cfg.NET_TYPE = "lidar"
        assert C.cfg.TEST.FRAME_GRAPHS is True
        C.cfg.TEST.NMS_THRESH = FRAME_NMS_THRESH
        net = lidarnet(num_layers=101)
        net.create_architecture(2, tag="default", anchor_scales=C.cfg.LIDAR.ANCHOR_SCALES[0],
                                anchor_ratios=C.cfg.LIDAR.ANCHOR_ANGLES)
        net.load_state_dict(seeded_state_dict(net, FRAME_SEED, bn_mode="tame"), strict=True)
        net.eval()
        net._device = DEV
        net.to(DEV)
        rng = np.random.default_rng(3)
        blob = (rng.random((1, 208, 176, 15)) * (rng.random((1, 208, 176, 15)) < 0.05)).astype(np.float32)
        data = torch.from_numpy(blob).to(DEV)
        info = np.array([0, 176, 0, 208, 0, 12, 0.5], np.float32)
        max_out = int(C.cfg.TEST.RPN_POST_NMS_TOP_N)
        pool = net.frame_pool(streams=1, capture_after=1, autotune=False, warmup=1)
        records = {}
        for switch in (True, False):
            C.cfg.TEST.NMS_ROTATED = switch
            key = pool.key_of(data.shape, info, FRAME_THRESH, FRAME_MAX_DETS, max_out)
            runner = pool.runner(data.shape, info, FRAME_THRESH, FRAME_MAX_DETS, max_out)
            assert runner is not None and runner.graph is not None
            dets, cnt = runner.run(data, poison=True)
            torch.cuda.synchronize()
            e_dets, e_cnt = detect_frame_device(net, data, info, FRAME_THRESH, FRAME_MAX_DETS, max_out)
            p = net._predictions
            n = int(p["rois_count"].item())
            records[switch] = dict(key=key, dets=dets.cpu().numpy().copy(), cnt=cnt.cpu().numpy().copy(),
                                   e_dets=e_dets.cpu().numpy(), e_cnt=e_cnt.cpu().numpy(), n=n,
                                   cp=p["cls_prob"].cpu().numpy().copy(), pb=p["pred_boxes"].cpu().numpy().copy(),
                                   yaw_less=[t.cpu().numpy() for t in ops.filter_per_class_lidar(
                                       p["pred_boxes"], p["cls_prob"], FRAME_THRESH, C.cfg.TEST.NMS_THRESH, FRAME_MAX_DETS,
                                       max_out, roi_count=p["rois_count"])])
        on, off = records[True], records[False]
        assert on["key"] != off["key"] and pool.stats["captures"] == 2 and pool.stats["eager"] == 0, pool.stats
        for r in (on, off):                                            # replay == eager, bit for bit
            assert r["dets"].tobytes() == r["e_dets"].tobytes() and r["cnt"].tobytes() == r["e_cnt"].tobytes()
        # the second frame follows the new setting: the yaw-less filter on its own cls_prob / pred_boxes
        assert off["dets"].tobytes() == off["yaw_less"][0].tobytes() and off["cnt"].tobytes() == off["yaw_less"][1].tobytes()
        # the first frame: the host reference of the rotated rule on the frame's eager cls_prob / pred_boxes
        ref = host_filter(on["pb"], on["cp"], on["n"], FRAME_THRESH, float(C.cfg.TEST.NMS_THRESH), FRAME_MAX_DETS)
        kept, cut, margin = ref[1]
        print("frame: %d RoIs, %d kept by the rotated rule, %d after max_dets, margin %.3e; yaw-less keeps %d"
              % (on["n"], len(kept), len(cut), margin, int(on["yaw_less"][1][1])))
        assert margin > MARGIN, "a pair within 1e-6 of the threshold: pick another seed"
        assert 0 < len(cut) < on["n"] and int(off["cnt"][1]) != len(cut), "the frame does not tell the two rules apart"
        want = np.zeros_like(on["e_dets"])
        want[1, :len(cut), :7] = on["pb"][cut, 7:14]
        want[1, :len(cut), 7] = on["cp"][cut, 1]
        np.testing.assert_array_equal(on["e_cnt"], [0, len(cut)])
        np.testing.assert_array_equal(on["e_dets"], want)
    finally:
        C.reset_cfg()
