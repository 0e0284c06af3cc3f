"""The COCO evaluator's host path (datasets/coco_eval.py, ``device=None``) against values worked out by hand - they depend on
no restatement - and the vectorised tail against the loops of tests/coco_restatement.py.  All boxes are [x, y, w, h]; each
hand case is one image and one category; the parameters are the defaults.  Stats order: AP, AP50, AP75, AP small / medium /
large, AR@1 / @10 / @100, AR small / medium / large."""
import functools
import json
import os
import pickle

import numpy as np
import pytest

import coco_restatement as R
import coco_scenes as S
from faster_rcnn_pytorch_multimodal_amd.datasets import coco_eval as C

AP, AP50, AP75, AP_S, AP_M, AP_L, AR1, AR10, AR100, AR_S, AR_M, AR_L = range(12)


def eq(value, want):
    """A precision is tp / (fp + tp + np.spacing(1)): a hand value of 1 comes out as 1 - 2.2e-16, and a mean over the ten
    thresholds adds a few roundings.  1e-12 is far above that and far below any other outcome (the nearest is a multiple
    of 1/101 away)."""
    return abs(value - want) <= 1e-12


@functools.lru_cache(maxsize=None)
def hand(name):
    gt, res = S.hand_cases()[name]
    return C.evaluate(gt, res)


@functools.lru_cache(maxsize=None)
def scene_result(seed=0):
    gt, res = S.seeded_scene(seed)
    return C.evaluate(gt, res)


def test_identical_box():
    s = hand('identical')['stats']
    assert eq(s[AP], 1) and eq(s[AP50], 1) and eq(s[AP75], 1)
    assert eq(s[AP_M], 1.0) and s[AP_S] == -1.0 and s[AP_L] == -1.0
    assert eq(s[AR1], 1.0)


def test_iou_exactly_077():
    r = hand('iou_077')
    assert r['ious'].tolist() == [0.77]
    s = r['stats']
    assert eq(s[AP], 0.6) and eq(s[AP50], 1.0) and eq(s[AP75], 1.0)
    assert eq(s[AR100], 0.6) and eq(s[AP_L], 0.6)


def test_crowd_absorbs_detections():
    r = hand('crowd')
    assert eq(r['stats'][AP], 0.5)                      # 1/3 if either of the first two detections counted as a false positive
    assert (r['dt_match'][0] == 1).all() and (r['dt_match'][1] == 1).all()        # the crowd box, at every (a, t)
    assert r['dt_ignore'][0].all() and r['dt_ignore'][1].all()
    ov = r['ious'].reshape(4, 2)
    assert ov[0, 1] == 1.0 and ov[1, 1] == 1.0        # the union is the detection's own area
    assert (r['dt_match'][3, 0] == 0).all() and (r['dt_match'][2] == -1).all()


def test_area_range():
    s = hand('area_range')['stats']
    assert eq(s[AP], 0.5) and eq(s[AP_S], 1.0) and s[AP_L] == -1.0


def test_max_dets():
    s = hand('max_dets')['stats']
    assert eq(s[AR1], 0.5) and eq(s[AR10], 1.0)


def test_threshold_equality_and_tie_rule():
    r = hand('threshold')
    assert r['ious'].tolist() == [0.5]
    s = r['stats']
    assert eq(s[AP50], 1.0) and eq(s[AP75], 0.0) and eq(s[AP], 0.1)
    t = hand('tie')
    assert t['ious'].tolist() == [0.5, 0.5]
    assert t['dt_match'][0, 0, 0] == 1                # the later of two boxes with equal overlap, at t = 0.5
    assert (t['dt_match'][0, 0, 1:] == -1).all()


def test_boundaries():
    r = hand('boundaries')
    labels = r['params'].area_lbl
    small, medium = labels.index('small'), labels.index('medium')
    assert not r['gt_ignore'][0, small] and not r['gt_ignore'][0, medium]         # area 1024 = 32 * 32
    assert not r['gt_ignore'][1, small] and not r['gt_ignore'][1, medium]         # `area` 1024 although w*h = 1600
    assert r['gt_ignore'][2, small] and not r['gt_ignore'][2, medium]             # `area` 5000 although w*h = 100
    g = C.load_ground_truth(S.hand_cases()['boundaries'][0])
    assert g.get(1, 1)['area'].tolist() == [1024.0, 1024.0, 5000.0]
    assert g.get(1, 1)['bbox'].tolist()[1] == [100, 0, 40, 40]
    assert g.get(1, 1)['iscrowd'].tolist() == [False, False, False]


def test_loader_keeps_the_100_highest_scores_ties_in_file_order():
    rng = np.random.default_rng(3)
    scores = np.round(rng.uniform(.1, 1, 130), 1)                                 # ten distinct values: many ties
    gt = S.annotations([1], [1], [(1, 1, [0, 0, 10, 10], 0)])
    res = S.results([(1, 1, [i, 0, 10, 10], float(s)) for i, s in enumerate(scores)])
    r = C.evaluate(gt, res)
    want = sorted(range(130), key=lambda i: (-scores[i], i))[:100]
    assert r['det_index'].tolist() == want
    assert r['det_scores'].tolist() == [scores[i] for i in want]
    assert r['det'][:, 0].tolist() == [float(i) for i in want]


def test_loader_rules():
    gt = S.annotations([1, 2], [1, 2], [(1, 1, [0, 0, 10, 10], 0)])
    good = (1, 1, [0, 0, 10, 10], .5)
    with pytest.raises(ValueError):
        C.evaluate(gt, S.results([good, (3, 1, [0, 0, 10, 10], .5)]))            # unknown image
    with pytest.raises(ValueError):
        C.load_results(S.results([(3, 1, [0, 0, 10, 10], .5)]), gt)
    kept = C.load_results(S.results([good, (1, 5, [0, 0, 10, 10], .9)]), gt)      # unknown category: dropped
    assert len(kept) == 1 and kept.category_id.tolist() == [1]
    assert C.evaluate(gt, S.results([good, (1, 5, [0, 0, 10, 10], .9)]))['stats'][0] > 1 - 1e-12
    for bad in ((1, 1, [0, float('nan'), 10, 10], .5), (1, 1, [0, 0, float('inf'), 10], .5), (1, 1, [0, 0, 10, 10], float('nan'))):
        with pytest.raises(ValueError):
            C.load_results(S.results([good, bad]))
    assert kept.area.tolist() == [100.0]


def test_results_file_and_printing(tmp_path, capsys):
    classes = ('__background__', 'cat', 'dog')
    class_to_cat_id = {'cat': 7, 'dog': 9}
    image_ids = [11, 12]
    all_boxes = [[np.zeros((1, 5)), np.zeros((1, 5))],                            # class 0 is skipped
                 [np.array([[10., 20., 59., 69., .9]]), []],
                 [np.zeros((0, 5)), np.array([[0., 0., 9., 9., .8], [100., 100., 109., 119., .7]])]]
    res_file = str(tmp_path / 'res.json')
    C.write_coco_results_file(all_boxes, image_ids, classes, class_to_cat_id, res_file)
    with open(res_file) as f:
        raw = json.load(f)
    assert raw == [{'image_id': 11, 'category_id': 7, 'bbox': [10.0, 20.0, 50.0, 50.0], 'score': .9},
                   {'image_id': 12, 'category_id': 9, 'bbox': [0.0, 0.0, 10.0, 10.0], 'score': .8},
                   {'image_id': 12, 'category_id': 9, 'bbox': [100.0, 100.0, 10.0, 20.0], 'score': .7}]
    back = C.load_results(res_file)
    assert back.bbox.tolist() == [x['bbox'] for x in raw] and back.score.tolist() == [.9, .8, .7]
    gt = S.annotations(image_ids, [7, 9], [(11, 7, [10, 20, 50, 50], 0), (12, 9, [0, 0, 10, 10], 0)])
    out = C.evaluate_detections(all_boxes, image_ids, classes, class_to_cat_id, gt, str(tmp_path))
    with open(os.path.join(str(tmp_path), 'detection_results.pkl'), 'rb') as f:
        loaded = pickle.load(f)
    assert np.array_equal(loaded['precision'], out['precision']) and np.array_equal(loaded['stats'], out['stats'])
    capsys.readouterr()
    lines = C.print_detection_eval_metrics(out, classes)
    printed = capsys.readouterr().out.splitlines()
    assert printed == lines
    head = lines.index('~~~~ Summary metrics ~~~~')
    assert lines[1:head] == ['100.0', '100.0', '100.0']                           # overall, then one line per foreground class
    assert lines[head + 1:] == C.summarize(out) and len(C.summarize(out)) == 12
    assert lines[head + 1] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000'
    assert lines[head + 7] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 1.000'


def test_scene_meets_its_conditions():
    cond = S.scene_conditions(scene_result())
    assert all(cond.values()), cond


def test_scene_contents():
    r = scene_result()
    n_det, n_gt = np.diff(r['det_offsets']), np.diff(r['gt_offsets'])
    assert ((n_gt == 0) & (n_det > 0)).any() and ((n_gt > 0) & (n_det == 0)).any()
    assert S.EMPTY_IMAGE not in r['pair_image'].tolist()
    big = (r['pair_image'] == S.BIG_PAIR[0]) & (r['pair_category'] == S.BIG_PAIR[1])
    assert n_det[big].tolist() == [100]               # 130 in the file
    assert n_gt.max() >= 12 and 0.08 < r['gt_crowd'].mean() < 0.25
    assert (r['gt'][:, 4] == 1024).any() and (r['gt'][:, 4] == 9216).any()
    assert len(np.unique(r['det_scores'])) < len(r['det_scores']) / 4             # ties


@pytest.mark.parametrize('seed', [0, 1])
def test_vectorised_tail_equals_the_restated_loops(seed):
    r = scene_result(seed)
    params = r['params']
    want_p, want_r, want_s = R.accumulate(r, params)
    got_p, got_r, got_s = C.accumulate(r, params)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_r, want_r) and np.array_equal(got_s, want_s)
    assert np.array_equal(C.compute_stats(got_p, got_r, params), R.stats(want_p, want_r, params))
    # and the host path's own loops say the same
    assert np.array_equal(r['precision'], want_p) and np.array_equal(r['recall'], want_r)
    assert np.array_equal(r['scores'], want_s) and np.array_equal(r['stats'], R.stats(want_p, want_r, params))
    assert (want_p > -1).any() and 0 < r['stats'][0] < 1


def test_tail_with_other_parameters():
    gt, res = S.seeded_scene(0)
    params = C.Params(iou_thrs=np.linspace(.15, .95, 17), rec_thrs=np.linspace(0, 1, 11), max_dets=(2, 5),
                      area_rng=((0, 1e10), (0, 500), (500, 1e10)), area_lbl=('all', 'small', 'large'))
    r = C.evaluate(gt, res, params)
    want = R.accumulate(r, params)
    got = C.accumulate(r, params)
    for g, w, h in zip(got, want, (r['precision'], r['recall'], r['scores'])):
        assert g.shape == w.shape and np.array_equal(g, w) and np.array_equal(h, w)
    assert r['precision'].shape == (17, 11, 6, 3, 2) and np.diff(r['det_offsets']).max() == 5
    assert r['stats'][4] == -1.0                      # no 'medium' label in these parameters
