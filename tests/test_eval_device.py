"""``frcnn_eval_match`` and the ``device='cuda'`` branch of the evaluators against the package's float64 HOST path
(``waymo_eval.iou`` and the host loops; tests/eval_scenes.py records the host walk) - never against the device code.

Overlap tolerance.  The kernel restates ``iou`` term for term in float64 with contraction off; what differs is the
device's cos / sin of ``ry`` and numpy's ``np.dot`` (BLAS: its own summation and fused multiply-adds) in the shoelace
sum.  The largest absolute difference over the hand-built pairs and the seeded scenes of this file, measured on an
MI355X, is ``MEASURED_GAP`` (profiles/device_eval.md); the tests assert 16 x that value, which must stay below 1e-9.
Matching is exact: the scenes are checked (from the HOST overlaps) to hold no overlap within 1e-6 of a threshold."""
import functools
import os

import numpy as np
import pytest

import eval_scenes as S
from faster_rcnn_pytorch_multimodal_amd import _hip
from faster_rcnn_pytorch_multimodal_amd.datasets import cadc_eval as Cd
from faster_rcnn_pytorch_multimodal_amd.datasets import device_eval as D
from faster_rcnn_pytorch_multimodal_amd.datasets import kitti_eval as K
from faster_rcnn_pytorch_multimodal_amd.datasets import waymo_eval as Wm

pytestmark = pytest.mark.gpu

MEASURED_GAP = 1.17e-12                  # largest |device - host| overlap (1.1624e-12, rounded up), profiles/device_eval.md
OV_BOUND = 16 * MEASURED_GAP
TYPES = ('2d', 'bev_aa', 'bev', '3d')


def test_the_asserted_bound_is_below_1e_9():
    assert 0 < OV_BOUND < 1e-9


def hand_pairs():
    """(detection, gt) 7-element pairs: identical boxes (IoU 1, collinear edges), edge-touching (zero-area intersection),
    full containment, a square against itself turned by pi/4 (8-vertex intersection), ry exactly 0, pi/2, pi, -pi,
    disjoint boxes, disjoint and touching height ranges."""
    sq = np.array([1.0, -2.0, 0.5, 2.0, 2.0, 2.0, 0.0])
    pairs = []
    for ry in (0.0, np.pi / 2, np.pi, -np.pi, np.pi / 4, 0.3):
        a = sq.copy()
        a[6] = ry
        pairs.append((a, a.copy()))                                          # identical
        for ry2 in (0.0, np.pi / 2, np.pi, -np.pi):
            b = sq.copy()
            b[6] = ry2
            pairs.append((a, b))
            for off in ((2.0, 0, 0), (0, 2.0, 0), (0.5, 0.25, 0), (7.0, 7.0, 0), (0, 0, 2.0), (0, 0, 3.0), (0.5, 0, 1.0)):
                c = b.copy()
                c[:3] += off                                                 # touching edge / overlap / disjoint / heights
                pairs.append((a, c))
            big = b.copy()
            big[3:6] = (6.0, 5.0, 4.0)                                       # containment, both ways
            pairs += [(a, big), (big, a)]
    long = np.array([0.0, 0.0, 0.0, 4.5, 1.8, 1.6, 0.7])
    pairs.append((long, long * np.array([1, 1, 1, 1, 1, 1, -1.0])))         # crossed boxes: 8-vertex intersection
    return pairs


def _device_pairs(eval_type, pairs):
    """One frame per pair (one detection, one gt box), through ops.eval_match: the device overlap of each pair."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    det = np.array([p[0] for p in pairs])
    gt = np.array([p[1] for p in pairs])
    if eval_type == '2d':
        det, gt = S.to_2d(det), S.to_2d(gt)
    n = len(pairs)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()

    off = up(np.arange(n + 1), np.int32)
    out = ops.eval_match(up(det, np.float64), up(np.arange(n), np.int32), off, up(gt, np.float64), up(np.zeros(n), np.uint8),
                         up(np.zeros(n), np.int32), off, eval_type, 0.5, max_gt_per_frame=1)
    host = np.array([Wm.iou(g[None], d, eval_type)[0] for d, g in zip(det, gt)])
    return out[2].cpu().numpy(), host, out


@pytest.mark.parametrize("eval_type", TYPES)
def test_overlaps_of_hand_built_pairs(hip, eval_type):
    dev, host, out = _device_pairs(eval_type, hand_pairs())
    gap = np.abs(dev - host).max()
    print("overlap gap %s hand-built pairs: %.3e" % (eval_type, gap))
    assert np.isfinite(host).all() and host.max() > 1 - 1e-12 and host.min() == 0.0
    assert gap <= OV_BOUND
    assert (out[1].cpu().numpy() == 0).all()                                 # jmax inside the frame


# ---- seeded scenes: matching ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_scene(seed, eval_type, ignore_dc=True, counts=S.GT_COUNTS):
    recs, tokens, conf, boxes = S.scene(seed, counts, eval_type)
    return recs, tokens, conf, boxes, S.host_overlaps(recs, tokens, conf, boxes, eval_type, ignore_dc)


def _compare(recs, tokens, conf, boxes, visits, eval_type, ovthresh, ignore_dc, label=""):
    host = S.host_walk(recs, visits, len(tokens), ovthresh)
    host_hit = [r['hit'].copy() for r in recs]
    for r in recs:
        r['hit'][:] = True                                                    # the device path must rewrite every flag
    row_of_det, code, jmax, ovmax, ovmax_dc = D.match_detections(tokens, conf, boxes, recs, ovthresh, eval_type, ignore_dc)
    finite = np.isfinite(host['ovmax'])
    gap = max(np.abs(ovmax[finite] - host['ovmax'][finite]).max() if finite.any() else 0.0,
              np.abs(ovmax_dc - host['ovmax_dc']).max() if len(ovmax_dc) else 0.0)
    print("overlap gap %s %s: %.3e" % (eval_type, label, gap))
    np.testing.assert_array_equal(row_of_det, host['row_of_det'])
    np.testing.assert_array_equal(code, host['code'])
    np.testing.assert_array_equal(jmax, host['jmax'])
    np.testing.assert_array_equal(ovmax[~finite], host['ovmax'][~finite])    # -inf in a frame without gt
    assert gap <= OV_BOUND
    for r, h in zip(recs, host_hit):
        np.testing.assert_array_equal(r['hit'], h)
    return host, gap


@pytest.mark.parametrize("eval_type", TYPES)
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_matching_on_seeded_scenes(hip, seed, eval_type):
    recs, tokens, conf, boxes, visits = _host_scene(seed, eval_type)
    assert S.threshold_margin(visits, (0.5, 0.7)) > 1e-6                     # no pair sits on a threshold
    seen = set()
    for ovthresh in (0.5, 0.7):
        host, _ = _compare(recs, tokens, conf, boxes, visits, eval_type, ovthresh, True, "seed %d" % seed)
        seen |= set(host['code'].tolist())
    assert seen == {S.NONE, S.TP, S.DUP_FP, S.FP}


@pytest.mark.parametrize("eval_type", ['2d', '3d'])
def test_ignore_dc_off(hip, eval_type):
    recs, tokens, conf, boxes = S.scene(1, S.GT_COUNTS, eval_type)
    visits = S.host_overlaps(recs, tokens, conf, boxes, eval_type, False)
    assert S.threshold_margin(visits, (0.5,)) > 1e-6
    off, _ = _compare(recs, tokens, conf, boxes, visits, eval_type, 0.5, False, "dc off")
    on = S.host_walk(recs, _host_scene(1, eval_type)[4], len(tokens), 0.5)
    assert (off['ovmax_dc'] == 0).all() and (off['code'] != on['code']).any()


# ---- edge cases ------------------------------------------------------------------------------------------------------------
def _small(dets, recs, eval_type='bev', ovthresh=0.5, ignore_dc=True, conf=None):
    tokens = [d[0] for d in dets]
    boxes = np.array([d[1] for d in dets], dtype=np.float64).reshape(len(dets), 7)
    conf = np.linspace(0.9, 0.1, len(dets)) if conf is None else np.asarray(conf, dtype=np.float64)
    visits = S.host_overlaps(recs, tokens, conf, boxes, eval_type, ignore_dc)
    assert S.threshold_margin(visits, (ovthresh,)) > 1e-6
    return _compare(recs, tokens, conf, boxes, visits, eval_type, ovthresh, ignore_dc, "edge case")[0]


BOX = np.array([3.0, 4.0, 0.0, 4.0, 2.0, 1.5, 0.4])


def test_two_identical_gt_boxes_first_index_wins(hip):
    recs = [Wm.make_rec("f", [BOX + 20, BOX, BOX], difficulty=[0, 1, 2])]
    host = _small([("f", BOX), ("f", BOX)], recs, '3d')
    assert host['jmax'].tolist() == [1, 1] and host['code'].tolist() == [S.TP, S.DUP_FP]
    assert recs[0]['hit'].tolist() == [False, True, False]


def test_equal_confidence_keeps_numpys_order(hip):
    recs = [Wm.make_rec("f", [BOX], difficulty=[0]), Wm.make_rec("g", [BOX], difficulty=[0])]
    dets = [("g", BOX), ("f", BOX), ("f", BOX * 1.01), ("f", BOX * 0.99), ("g", BOX * 1.01)]
    host = _small(dets, recs, 'bev', conf=[0.5] * 5)
    assert sorted(host['code'].tolist()) == [S.TP, S.TP, S.DUP_FP, S.DUP_FP, S.DUP_FP]


def test_tokens_without_a_record_consume_no_row_and_frames_without_gt_count_nothing(hip):
    recs = [Wm.make_rec("f", [BOX], difficulty=[0]), Wm.make_rec("skipped", [BOX], ignore_frame=True),
            Wm.make_rec("empty", np.zeros((0, 7)), ignore_frame=False), Wm.make_rec("f", [BOX + 50])]
    dets = [("nowhere", BOX), ("skipped", BOX), ("empty", BOX), ("f", BOX), ("f", BOX + 9)]
    host = _small(dets, recs)
    assert host['row_of_det'].tolist() == [-1, -1, 0, 1, 2] and host['code'].tolist() == [S.NONE, S.TP, S.FP]
    assert host['ovmax'][0] == -np.inf and not recs[1]['hit'].any() and not recs[3]['hit'].any()


def test_empty_detections_file(hip):
    recs = [Wm.make_rec("f", [BOX], difficulty=[0])]
    recs[0]['hit'][:] = True
    row_of_det, code, jmax, ovmax, ovmax_dc = D.match_detections([], np.zeros(0), np.zeros((0, 7)), recs, 0.5, 'bev', True)
    assert row_of_det.shape == code.shape == jmax.shape == ovmax.shape == ovmax_dc.shape == (0,)
    assert not recs[0]['hit'].any()
    row_of_det, code, _, _, _ = D.match_detections(["f"], np.ones(1), BOX[None], [], 0.5, 'bev', True)
    assert row_of_det.tolist() == [-1] and code.shape == (0,)


@pytest.mark.parametrize("n_det", [256, 257])
def test_one_frame_with_a_full_tile_of_detections_and_one_more(hip, n_det):
    rng = np.random.default_rng(n_det)
    gt = S.random_boxes(rng, 6)
    det = np.concatenate([S.jitter(rng, gt[rng.integers(0, 6, n_det - 10)]), S.random_boxes(rng, 10)])
    recs = [Wm.make_rec("f", gt, difficulty=rng.integers(0, 3, 6), ignore=[0, 0, 1, 0, 0, 0], boxes_dc=S.random_boxes(rng, 2))]
    host = _small([("f", d) for d in det], recs, '3d', conf=rng.uniform(0, 1, n_det))
    assert (host['code'] == S.TP).sum() == 5 and (host["code"] == S.DUP_FP).sum() > 20


def test_a_frame_beyond_the_lds_resident_gt_count(hip):
    from faster_rcnn_pytorch_multimodal_amd import ops
    rng = np.random.default_rng(7)
    n_gt = ops.EVAL_LDS_GT + 1
    assert n_gt == 2049 and _hip.load().frcnn_eval_match_ws_bytes(n_gt + 1, n_gt) == 4 * (n_gt + 1)
    assert _hip.load().frcnn_eval_match_ws_bytes(n_gt + 1, ops.EVAL_LDS_GT) == 0
    gt = S.random_boxes(rng, n_gt)
    gt[:, :2] = rng.uniform(-400, 400, (n_gt, 2))
    recs = [Wm.make_rec("small", [BOX], difficulty=[0]), Wm.make_rec("big", gt, difficulty=rng.integers(0, 3, n_gt))]
    dets = [("big", S.jitter(rng, gt[2048:2049])[0]), ("small", BOX), ("big", gt[2048]), ("big", S.jitter(rng, gt[5:6])[0])]
    host = _small(dets, recs)
    assert host['jmax'].tolist() == [2048, 0, 2048, 5] and host['code'].tolist() == [S.TP, S.TP, S.DUP_FP, S.TP]
    assert recs[1]['hit'].sum() == 2


# ---- evaluators --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn,d_levels,eval_type", [(Wm.waymo_eval, 2, '3d'), (K.kitti_eval, 3, 'bev'), (Cd.cadc_eval, 2, '2d'),
                                                   (Cd.cadc_eval, 3, 'bev_aa')])
def test_evaluators_device_branch_equals_their_host_branch(hip, tmp_path, fn, d_levels, eval_type):
    recs, tokens, conf, boxes, visits = _host_scene(2, eval_type)
    assert S.threshold_margin(visits, (0.7,)) > 1e-6
    tokens = list(tokens)
    tokens[3] = "no_such_frame.bin"
    path = os.path.join(str(tmp_path), "det.txt")
    S.write_detfile(path, tokens, conf, boxes)
    elem = boxes.shape[1]
    host_recs = [dict(r, hit=r['hit'].copy()) for r in recs]
    h1, h2, h3, host = fn(path, host_recs, 0.7, eval_type, d_levels, bbox_elem=elem, ignore_dc=True)
    d1, d2, d3, dev = fn(path, recs, 0.7, eval_type, d_levels, bbox_elem=elem, ignore_dc=True, device='cuda')
    assert d1 is d2 is d3 and d1 is not dev['ap']                              # the three-way alias is kept
    for key in ('tp', 'fp', 'npos'):
        np.testing.assert_array_equal(dev[key], host[key])
    assert host['tp'].sum() > 10 and host['fp'].sum() > 10
    for key in ('ap', 'mean_recall', 'mean_precision'):
        assert np.abs(dev[key] - host[key]).max() <= 1e-12
    assert np.abs(d1 - h1).max() <= 1e-12
    for r, h in zip(recs, host_recs):
        np.testing.assert_array_equal(r['hit'], h['hit'])
    rows = int(dev['code'].shape[0])
    assert rows == len(tokens) - 1 and dev['jmax'].shape == dev['ovmax'].shape == (rows,)


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_value_errors(hip):
    recs = [Wm.make_rec("f", [BOX], difficulty=[0])]
    for col, value in ((3, 0.0), (4, -2.0), (5, 0.0), (1, np.nan), (6, np.inf)):
        bad = BOX.copy()
        bad[col] = value
        for eval_type in ('bev', 'bev_aa', '3d'):
            with pytest.raises(ValueError):
                D.match_detections(["f"], np.ones(1), bad[None], recs, 0.5, eval_type, True)
    with pytest.raises(ValueError):
        D.match_detections(["f"], np.ones(1), BOX[None], recs, 0.5, 'sphere', True)
    with pytest.raises(ValueError):
        K.kitti_eval("unused", recs, 0.5, 'bev', 2, bbox_elem=7, device='cuda')


def test_hip_errors_of_the_op(hip):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    dev = "cuda"
    det, gt = torch.zeros(2, 7, dtype=torch.float64, device=dev), torch.zeros(3, 7, dtype=torch.float64, device=dev)
    rows, off_d = torch.arange(2, dtype=torch.int32, device=dev), torch.tensor([0, 2], dtype=torch.int32, device=dev)
    ign, dif = torch.zeros(3, dtype=torch.uint8, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    off_g = torch.tensor([0, 3], dtype=torch.int32, device=dev)
    good = [det, rows, off_d, gt, ign, dif, off_g, 'bev', 0.5]
    bad = {0: det.float(), 1: rows.long(), 2: off_d.cpu(), 3: gt[:, :4].contiguous(), 4: ign.int(), 5: dif[:2], 6: off_g[:1],
           7: 'sphere'}
    for pos, value in bad.items():
        args = list(good)
        args[pos] = value
        with pytest.raises(_hip.HipError):
            ops.eval_match(*args)
    with pytest.raises(_hip.HipError):
        ops.eval_match(*good, dc_boxes=gt)                                     # don't-care boxes without offsets
    with pytest.raises(_hip.HipError):
        ops.eval_match(det[:, :4].contiguous(), rows, off_d, gt, ign, dif, off_g, '2d', 0.5)
    lib = _hip.load()
    rc = lib.frcnn_eval_match(det.data_ptr(), rows.data_ptr(), off_d.data_ptr(), 2, gt.data_ptr(), ign.data_ptr(),
                              dif.data_ptr(), off_g.data_ptr(), 3, None, None, 0, 1, 2, 0.5, 0.5, 4000, None, None, None, None,
                              None, None, None, 0, None)
    assert rc == -1 and b"null detection array" in lib.frcnn_last_error()
    out = [torch.zeros(2, dtype=torch.int32, device=dev) for _ in range(5)]
    rc = lib.frcnn_eval_match(det.data_ptr(), rows.data_ptr(), off_d.data_ptr(), 2, gt.data_ptr(), ign.data_ptr(),
                              dif.data_ptr(), off_g.data_ptr(), 3, None, None, 0, 1, 2, 0.5, 0.5, 4000, out[0].data_ptr(),
                              out[1].data_ptr(), det.data_ptr(), det.data_ptr(), out[2].data_ptr(), ign.data_ptr(), None, 0,
                              None)
    assert rc == -2 and b"workspace" in lib.frcnn_last_error()                 # a frame above the LDS count needs ws
    rc = lib.frcnn_eval_match(None, None, off_d.data_ptr(), 0, None, None, None, off_g.data_ptr(), 0, None, None, 0, 1, 7, 0.5,
                              0.5, 0, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"eval_type" in lib.frcnn_last_error()
