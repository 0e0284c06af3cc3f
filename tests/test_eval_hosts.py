"""Host side of the KITTI / CADC evaluators and of the device scoring path (no GPU): the ``kitti_eval`` / ``cadc_eval`` host
loops on known-answer cases (lib/datasets/kitti_eval.py:116-215,271-282, cadc_eval.py:172-205,252-264), their agreement with
``waymo_eval`` under a shift of the difficulties, ``device_eval.prepare`` (token map, rows, CSR) against the host loop's
visiting order, and the vectorised tail against the ``sorted(zip(...))`` tail."""
import os

import numpy as np
import pytest

import eval_scenes as S
from faster_rcnn_pytorch_multimodal_amd.datasets import cadc_eval as Cd
from faster_rcnn_pytorch_multimodal_amd.datasets import device_eval as D
from faster_rcnn_pytorch_multimodal_amd.datasets import kitti_eval as K
from faster_rcnn_pytorch_multimodal_amd.datasets import waymo_eval as Wm


def _box(x, y, size=100.0):
    return [x, y, x + size, y + size]


def _known_case(tmp_path):
    """Two frames.  a.png: gt 0 easy, gt 1 hard, gt 2 ignored.  b.png: one moderate gt, one don't-care box.
    Detections by descending score: hit gt 0 (tp), hit gt 0 again (duplicate), hit gt 1 (tp at level 2 only), hit the
    ignored gt (nothing), clutter (fp everywhere), a box on the don't-care region of b (dropped when ignore_dc), hit b's gt."""
    recs = [Wm.make_rec("a.png", [_box(0, 0), _box(300, 0), _box(600, 0)], difficulty=[0, 2, 0], ignore=[0, 0, 1]),
            Wm.make_rec("b.png", [_box(0, 0)], difficulty=[1], boxes_dc=[_box(500, 500)])]
    dets = [("a.png", 0.95, _box(2, 1)), ("a.png", 0.90, _box(-3, 2)), ("a.png", 0.85, _box(301, 1)),
            ("a.png", 0.80, _box(601, -1)), ("a.png", 0.70, _box(300, 600)), ("b.png", 0.60, _box(503, 498)),
            ("b.png", 0.50, _box(1, 1))]
    path = os.path.join(str(tmp_path), "det.txt")
    S.write_detfile(path, [d[0] for d in dets], [d[1] for d in dets], [d[2] for d in dets])
    return path, recs


@pytest.mark.parametrize("fn", [K.kitti_eval, Cd.cadc_eval])
def test_level_rule_duplicates_and_dont_care(tmp_path, fn):
    path, recs = _known_case(tmp_path)
    mrec, mprec, m, plain = fn(path, recs, 0.5, '2d', 3, bbox_elem=4, ignore_dc=True)
    assert mrec is mprec is m and np.array_equal(m, plain['ap'])
    np.testing.assert_array_equal(plain['npos'], [[1, 1, 2], [0, 1, 1]])          # difficulty <= lvl, ignored box left out
    np.testing.assert_array_equal(plain['tp'], [[1, 1, 1], [0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 1, 1]])
    # the duplicate is a false positive at the SAME levels as its box, clutter at every level, the don't-care hit nowhere
    np.testing.assert_array_equal(plain['fp'], [[0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(recs[0]['hit'], [True, True, False])
    _, _, _, off = fn(path, recs, 0.5, '2d', 3, bbox_elem=4, ignore_dc=False)
    np.testing.assert_array_equal(off['fp'][5], [1, 1, 1])                         # not consulted: plain clutter


def test_d_levels_guards(tmp_path):
    path, recs = _known_case(tmp_path)
    for bad in (0, 1, 2, 4):
        with pytest.raises(ValueError):
            K.kitti_eval(path, recs, 0.5, '2d', bad, bbox_elem=4, ignore_dc=True)
    full = Cd.cadc_eval(path, recs, 0.5, '2d', 3, bbox_elem=4, ignore_dc=True)[3]
    for d_levels in (1, 2):
        _, _, m, plain = Cd.cadc_eval(path, recs, 0.5, '2d', d_levels, bbox_elem=4, ignore_dc=True)
        assert m.shape == (d_levels,)
        for key in ('tp', 'fp', 'npos'):
            np.testing.assert_array_equal(plain[key], full[key][:, :d_levels])
        np.testing.assert_array_equal(plain['ap'], full['ap'][:d_levels])
    four = Cd.cadc_eval(path, recs, 0.5, '2d', 4, bbox_elem=4, ignore_dc=True)[3]
    assert not four['tp'][:, 3].any() and not four['fp'][:, 3].any() and not four['npos'][:, 3].any()


@pytest.mark.parametrize("fn", [K.kitti_eval, Cd.cadc_eval])
@pytest.mark.parametrize("eval_type", ['2d', 'bev'])
def test_agrees_with_waymo_eval_when_difficulties_shift_by_one(tmp_path, fn, eval_type):
    """waymo counts ``difficulty <= lvl + 1`` over levels 0..1, kitti / cadc ``difficulty <= lvl`` over 0..2: with every
    difficulty one higher, waymo's two columns are the first two of the three."""
    recs, tokens, conf, boxes = S.scene(1, (0, 2, 7, 3), eval_type)
    path = os.path.join(str(tmp_path), "det.txt")
    S.write_detfile(path, tokens, conf, boxes)
    elem = boxes.shape[1]
    ours = fn(path, recs, 0.5, eval_type, 3, bbox_elem=elem, ignore_dc=True)[3]
    shifted = [dict(r, difficulty=r['difficulty'] + 1, hit=r['hit'].copy()) for r in recs]
    theirs = Wm.waymo_eval(path, shifted, 0.5, eval_type, 2, bbox_elem=elem, ignore_dc=True)[3]
    assert ours['tp'].sum() > 0 and ours['fp'].sum() > 0
    for key in ('tp', 'fp', 'npos', 'ap', 'mean_recall', 'mean_precision'):
        np.testing.assert_array_equal(ours[key][..., :2], theirs[key])


def test_empty_file_gives_zeros(tmp_path):
    path = os.path.join(str(tmp_path), "det.txt")
    open(path, 'w').close()
    recs = [Wm.make_rec("a.png", [_box(0, 0)], difficulty=[0])]
    for fn in (K.kitti_eval, Cd.cadc_eval):
        _, _, m, plain = fn(path, recs, 0.5, '2d', 3, bbox_elem=4, ignore_dc=False)
        assert not m.any() and plain['tp'].shape == (0, 3) and plain['npos'].sum() == 3


# ---- device_eval.prepare ------------------------------------------------------------------------------------------------
def test_token_map_is_find_rec():
    recs = [Wm.make_rec("a", [_box(0, 0)], ignore_frame=True), Wm.make_rec("a", [_box(5, 5)]), Wm.make_rec("a", [_box(9, 9)]),
            Wm.make_rec("b", []), Wm.make_rec("c", [], ignore_frame=False)]
    first = D.token_map(recs)
    for token in ("a", "b", "c", "missing"):
        rec = Wm.find_rec(recs, token)
        assert (rec is None) == (token not in first)
        if rec is not None:
            assert recs[first[token]] is rec
    assert first == {"a": 1, "c": 4}


@pytest.mark.parametrize("eval_type,ignore_dc", [('bev', True), ('3d', False), ('2d', True)])
def test_prepare_rows_and_csr_follow_the_host_visiting_order(eval_type, ignore_dc):
    recs, tokens, conf, boxes = S.scene(2, (0, 3, 5, 2), eval_type)
    recs[2]['ignore_frame'] = True                             # its detections consume no row
    tokens[4] = "no_such_frame.bin"
    conf[10:14] = 0.5                                          # ties: numpy's argsort order is the order
    visits = S.host_overlaps(recs, tokens, conf, boxes, eval_type, ignore_dc)
    host = S.host_walk(recs, visits, len(tokens), 0.5)
    p = D.prepare(tokens, conf, boxes, recs, eval_type, ignore_dc)
    np.testing.assert_array_equal(p.row_of_det, host['row_of_det'])
    assert (p.row_of_det == -1).sum() >= 2
    rows = int((p.row_of_det >= 0).sum())
    det_of_row = np.empty(rows, dtype=np.int64)
    det_of_row[p.row_of_det[p.row_of_det >= 0]] = np.nonzero(p.row_of_det >= 0)[0]
    assert p.det_offsets[0] == 0 and p.det_offsets[-1] == rows and len(p.det_offsets) == len(p.rec_of_frame) + 1
    for f, r in enumerate(p.rec_of_frame):
        rec = recs[r]
        lo, hi = p.det_offsets[f], p.det_offsets[f + 1]
        assert np.all(np.diff(p.det_rows[lo:hi]) > 0)                               # ascending rows inside a frame
        for slot in range(lo, hi):
            row = p.det_rows[slot]
            assert Wm.find_rec(recs, tokens[det_of_row[row]]) is rec and p.slot_of_row[row] == slot
            np.testing.assert_array_equal(p.det_boxes[slot], boxes[det_of_row[row]])
        g0, g1 = p.gt_offsets[f], p.gt_offsets[f + 1]
        np.testing.assert_array_equal(p.gt_boxes[g0:g1].reshape(rec['boxes'].shape), rec['boxes'])
        np.testing.assert_array_equal(p.gt_ignore[g0:g1].astype(bool), rec['ignore'])
        np.testing.assert_array_equal(p.gt_difficulty[g0:g1], rec['difficulty'])
        if ignore_dc:
            c0, c1 = p.dc_offsets[f], p.dc_offsets[f + 1]
            np.testing.assert_array_equal(p.dc_boxes[c0:c1].reshape(rec['boxes_dc'].shape), rec['boxes_dc'])
    assert (p.dc_boxes is None) == (not ignore_dc)
    assert sorted(p.det_rows.tolist()) == list(range(rows)) and p.max_gt_per_frame == 3
    assert [recs[r]['filename'] for r in p.rec_of_frame] == ["000000.bin", "000001.bin", "000003.bin"]


def test_prepare_rejects_what_the_host_path_cannot_score():
    recs, tokens, conf, boxes = S.scene(0, (2, 2), 'bev')
    for col, value in ((3, 0.0), (4, -1.0), (5, 0.0), (0, np.nan), (6, np.inf)):
        bad = boxes.copy()
        bad[1, col] = value
        with pytest.raises(ValueError):
            D.prepare(tokens, conf, bad, recs, 'bev', True)
    bad_recs = [dict(r, boxes=r['boxes'].copy()) for r in recs]
    bad_recs[0]['boxes'][0, 3] = 0.0
    with pytest.raises(ValueError):
        D.prepare(tokens, conf, boxes, bad_recs, '3d', False)
    with pytest.raises(ValueError):
        D.prepare(tokens, conf, boxes, recs, 'sphere', False)
    recs2, tokens2, conf2, boxes2 = S.scene(0, (2, 2), '2d')
    boxes2[0, 2] = boxes2[0, 0]                                 # a zero-width pixel box is legal under the +1 convention
    D.prepare(tokens2, conf2, boxes2, recs2, '2d', False)
    boxes2[0, 2] = np.inf
    with pytest.raises(ValueError):
        D.prepare(tokens2, conf2, boxes2, recs2, '2d', False)


def test_prepare_empty_file_and_no_records():
    recs, tokens, conf, boxes = S.scene(0, (2, 0), 'bev')
    p = D.prepare([], np.zeros(0), np.zeros((0, 7)), recs, 'bev', True)
    assert p.det_boxes.shape == (0, 7) and p.det_offsets.tolist() == [0, 0, 0] and p.gt_offsets.tolist() == [0, 2, 2]
    p = D.prepare(tokens, conf, boxes, [], 'bev', True)
    assert (p.row_of_det == -1).all() and p.rec_of_frame.size == 0 and p.det_offsets.tolist() == [0]


# ---- the vectorised tail ------------------------------------------------------------------------------------------------
def _loop_tail(tp, fp, npos, d_levels):
    """The evaluators' tail as written in waymo_eval (sorted(zip(...)))."""
    out = {'ap': np.zeros(d_levels), 'mean_recall': np.zeros(d_levels), 'mean_precision': np.zeros(d_levels)}
    fp_sum, tp_sum, npos_sum = np.cumsum(fp, axis=0), np.cumsum(tp, axis=0), np.sum(npos, axis=0)
    for i in range(d_levels):
        npos_d = npos_sum[i] if npos_sum[i] != 0 else 1.0
        rec_c = tp_sum[:, i] / float(npos_d)
        prec_c = tp_sum[:, i] / np.maximum(tp_sum[:, i] + fp_sum[:, i], np.finfo(np.float64).eps)
        if len(rec_c):
            rec_c, prec_c = zip(*sorted(zip(rec_c, prec_c)))
        out['mean_precision'][i] = np.average(prec_c) if len(prec_c) else 0.0
        out['mean_recall'][i] = np.average(rec_c) if len(rec_c) else 0.0
        out['ap'][i] = Wm.ap(rec_c, prec_c)
    return out


@pytest.mark.parametrize("n", [0, 1, 7, 500])
def test_vectorised_tail_equals_the_sorted_zip_tail(n):
    rng = np.random.default_rng(n)
    kind = rng.integers(0, 4, (n, 3))            # 0 / 3: nothing or a drop (equal-recall, equal-pair runs), 1 tp, 2 fp
    tp, fp = (kind == 1).astype(float), (kind == 2).astype(float)
    if n > 7:
        tp[40:60] = 0                            # a long run of equal recall with changing precision ...
        fp[40:60, 0] = 1
        tp[100:120], fp[100:120] = 0, 0          # ... and a run of identical pairs
    npos = np.array([[n // 2 + 1, 0, 3], [2, 0, 5]], dtype=float)   # a level without positives divides by 1
    want = _loop_tail(tp, fp, npos, 3)
    ap_d, mrec, mprec = D.ap_tail(tp, fp, npos, 3)
    np.testing.assert_array_equal(ap_d, want['ap'])
    np.testing.assert_array_equal(mrec, want['mean_recall'])
    np.testing.assert_array_equal(mprec, want['mean_precision'])


def test_scatter_tables_rules():
    m = {'code': np.array([S.TP, S.DUP_FP, S.FP, S.NONE, S.TP]), 'difficulty': np.array([0, 2, -1, -1, 3])}
    tp, fp = D.scatter_tables(6, 3, m, 0)                       # kitti / cadc: difficulty <= lvl
    np.testing.assert_array_equal(tp, [[1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(fp, [[0, 0, 0], [0, 0, 1], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
    tp, fp = D.scatter_tables(5, 2, m, 1)                       # waymo: difficulty <= lvl + 1
    np.testing.assert_array_equal(tp, [[1, 1], [0, 0], [0, 0], [0, 0], [0, 0]])
    np.testing.assert_array_equal(fp, [[0, 0], [0, 1], [1, 1], [0, 0], [0, 0]])
    tp, fp = D.scatter_tables(5, 4, m, 0)                       # cadc never writes a fourth column
    assert not tp[:, 3].any() and not fp[:, 3].any()


def test_python_constants_mirror_the_header():
    import re
    from faster_rcnn_pytorch_multimodal_amd import ops
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    header = open(os.path.join(root, "include", "frcnn_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define FRCNN_EVAL_([A-Z0-9_]+) (\d+)", header)}
    assert {t: defs[t.upper()] for t in ops.EVAL_TYPES} == ops.EVAL_TYPES
    assert (defs['NONE'], defs['TP'], defs['DUP_FP'], defs['FP']) == (ops.EVAL_NONE, ops.EVAL_TP, ops.EVAL_DUP_FP, ops.EVAL_FP)
    assert (S.NONE, S.TP, S.DUP_FP, S.FP) == (ops.EVAL_NONE, ops.EVAL_TP, ops.EVAL_DUP_FP, ops.EVAL_FP)
    assert (defs['CHUNK'], defs['LDS_GT']) == (ops.EVAL_CHUNK, ops.EVAL_LDS_GT)
    assert defs['CHUNK'] - 1 in S.GT_COUNTS and defs['CHUNK'] in S.GT_COUNTS and defs['CHUNK'] + 1 in S.GT_COUNTS
