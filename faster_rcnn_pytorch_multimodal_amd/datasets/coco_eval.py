"""COCO bbox evaluation, AP@[.50:.95] and the 12 summary numbers - counterpart of lib/datasets/coco.py:217-312 and of the
bbox part of ``pycocotools.COCOeval``, which the reference calls there.

PARITY UNPINNED against pycocotools: it is a compiled third-party extension, not a dependency of this package and absent
from the build and GPU machines.  The protocol below is restated from its published description; the tests pin it to
values worked out by hand (tests/test_coco_eval_host.py) and pin the device path to the host path (bit for bit,
tests/test_coco_eval_device.py).

Two paths, one result:
  * ``device=None``: the host path, the protocol as plain float64 loops (``match_host`` + ``accumulate_loops``).  It is
    the yardstick, not fast.
  * ``device='cuda'``: ``prepare`` on the host, ONE ``frcnn_coco_match`` launch for all pairs (csrc/coco_match.hip),
    read back, then the vectorised numpy tail ``accumulate``.

The protocol.
  Pairs      every (image, category) with at least one ground-truth box or one detection, images and categories in
             ascending id order.
  Detections of a pair: stable sort by descending score (ties keep results-file order), first ``max_dets[-1]`` kept.
  IoU        of detection d and ground truth g, both [x, y, w, h]: iw = min(dx+dw, gx+gw) - max(dx, gx), ih likewise;
             0 if iw <= 0 or ih <= 0; else i = iw*ih, u = dw*dh for a crowd g, dw*dh + gw*gh - i otherwise; i/u.  No +1.
  Area range a = [lo, hi]: a ground-truth box is IGNORED if it is crowd or its area is < lo or > hi (both ends inclusive);
             ground truth is visited non-ignored boxes first, each group in annotation order.
  Threshold t: walk the kept detections in score order.  best = min(t, 1 - 1e-10), m = none; over the ground truth in
             visiting order: skip g if it is already matched at this (a, t) and is not crowd; STOP if m is a non-ignored
             box and g is ignored; skip g if iou < best; otherwise best = iou, m = g (an IoU equal to the threshold
             matches, of two equal IoUs the later box wins).  A matched detection takes m's ignore flag; afterwards an
             UNMATCHED detection whose area is outside [lo, hi] is ignored.
  Accumulate per category k, area a, maxDet M: concatenate, over images in order, the first M detections of every pair of
             the category; stable sort by descending score; npig = number of non-ignored ground-truth boxes (0: leave
             -1); tp = matched & ~ignored, fp = ~matched & ~ignored, cumulative; rc = tp/npig, pr = tp/(fp+tp+spacing(1));
             recall = rc[-1] (0 with no detections); pr made non-increasing from the right; for every ``rec_thrs`` value
             pr and the score at np.searchsorted(rc, thr, side='left'), 0 past the end.
Out of scope: segmentation and keypoints, ``useCats = 0``, the dataset class (annotation indexing, roidb).
"""
import json
import os
import pickle

import numpy as np

RESULTS_PICKLE = 'detection_results.pkl'


class Params(object):
    """The evaluation parameters; all four are overridable.  The arrays are numpy's: the device takes them as they are."""

    def __init__(self, iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100), area_rng=None, area_lbl=None):
        self.iou_thrs = np.linspace(.5, .95, 10) if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
        self.rec_thrs = np.linspace(0, 1, 101) if rec_thrs is None else np.asarray(rec_thrs, dtype=np.float64).reshape(-1)
        self.max_dets = tuple(int(m) for m in max_dets)
        if area_rng is None:
            area_rng = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))
        self.area_rng = np.asarray(area_rng, dtype=np.float64).reshape(-1, 2)
        if area_lbl is None:
            area_lbl = ('all', 'small', 'medium', 'large')[:self.area_rng.shape[0]]
        self.area_lbl = tuple(area_lbl)
        if len(self.area_lbl) != self.area_rng.shape[0]:
            raise ValueError("%d area labels for %d area ranges" % (len(self.area_lbl), self.area_rng.shape[0]))
        if not self.iou_thrs.size or not self.rec_thrs.size or not self.max_dets or not self.area_rng.size:
            raise ValueError("empty parameter")
        if list(self.max_dets) != sorted(self.max_dets) or self.max_dets[0] < 1:
            raise ValueError("max_dets must ascend from at least 1, got %r" % (self.max_dets,))


class GroundTruth(object):
    """A COCO annotation set as flat arrays in annotation order.  ``image_ids`` / ``cat_ids``: ascending;
    ``img_index`` / ``cat_index`` index them per annotation; ``bbox`` (n, 4) [x, y, w, h], ``area`` (the annotation's
    field when present, else w*h), ``iscrowd``; ``ignore`` is ``iscrowd``."""

    def __init__(self, image_ids, cat_ids, img_index, cat_index, bbox, area, iscrowd):
        self.image_ids, self.cat_ids = image_ids, cat_ids
        self.img_index, self.cat_index = img_index, cat_index
        self.bbox, self.area, self.iscrowd = bbox, area, iscrowd

    @property
    def ignore(self):
        return self.iscrowd

    def get(self, image_id, cat_id):
        """{'bbox', 'area', 'iscrowd', 'ignore'} of one (image id, category id), annotation order."""
        sel = (self.image_ids[self.img_index] == image_id) & (self.cat_ids[self.cat_index] == cat_id)
        return {'bbox': self.bbox[sel], 'area': self.area[sel], 'iscrowd': self.iscrowd[sel], 'ignore': self.iscrowd[sel]}


class Results(object):
    """A results list as flat arrays in file order: ``image_id``, ``category_id``, ``bbox`` (n, 4), ``score``, ``area`` = w*h."""

    def __init__(self, image_id, category_id, bbox, score):
        self.image_id, self.category_id, self.bbox, self.score = image_id, category_id, bbox, score
        self.area = bbox[:, 2] * bbox[:, 3]

    def __len__(self):
        return self.score.shape[0]


def _ids(values, what):
    a = np.asarray(list(values))
    if a.size and a.dtype.kind not in 'iu':
        raise ValueError("%s ids must be integers" % what)
    return a.astype(np.int64).reshape(-1)


def _index_of(ids, sorted_ids):
    """Position of every id in ``sorted_ids`` and whether it is there."""
    if not sorted_ids.size:
        return np.zeros(ids.shape, dtype=np.int64), np.zeros(ids.shape, dtype=bool)
    pos = np.minimum(np.searchsorted(sorted_ids, ids), sorted_ids.size - 1)
    return pos, sorted_ids[pos] == ids


def load_ground_truth(path_or_dict):
    """A COCO annotation file or dict with ``images``, ``annotations`` and ``categories`` -> ``GroundTruth``."""
    if isinstance(path_or_dict, GroundTruth):
        return path_or_dict
    d = path_or_dict
    if not isinstance(d, dict):
        with open(d) as f:
            d = json.load(f)
    for key in ('images', 'annotations', 'categories'):
        if key not in d:
            raise ValueError("annotations without %r" % key)
    image_ids = np.unique(_ids((im['id'] for im in d['images']), 'image'))
    cat_ids = np.unique(_ids((c['id'] for c in d['categories']), 'category'))
    anns = d['annotations']
    n = len(anns)
    bbox = np.array([a['bbox'] for a in anns], dtype=np.float64).reshape(n, 4)
    area = np.array([a['area'] if 'area' in a else float(b[2]) * float(b[3]) for a, b in zip(anns, bbox)], dtype=np.float64)
    iscrowd = np.array([bool(a.get('iscrowd', 0)) for a in anns], dtype=bool)
    if not np.isfinite(bbox).all() or not np.isfinite(area).all():
        raise ValueError("ground truth: non-finite box or area")
    img_index, ok_i = _index_of(_ids((a['image_id'] for a in anns), 'image'), image_ids)
    cat_index, ok_c = _index_of(_ids((a['category_id'] for a in anns), 'category'), cat_ids)
    if not ok_i.all() or not ok_c.all():
        raise ValueError("an annotation names an image or a category that the file does not list")
    return GroundTruth(image_ids, cat_ids, img_index, cat_index, bbox, area, iscrowd)


def load_results(path_or_list, gt=None):
    """The results list of {'image_id', 'category_id', 'bbox': [x, y, w, h], 'score'} (or a file of it) -> ``Results``.
    A non-finite box or score raises ValueError.  With ``gt`` the ground truth's rules are applied here as well (they always
    are in ``evaluate``): a result whose image id is not among the ground truth's images raises ValueError, one whose
    category id is not among its categories is dropped, because the evaluated categories are the ground truth's."""
    r = path_or_list
    if not isinstance(r, Results):
        if not isinstance(r, (list, tuple)):
            with open(r) as f:
                r = json.load(f)
        n = len(r)
        bbox = np.array([x['bbox'] for x in r], dtype=np.float64).reshape(n, 4)
        score = np.array([x['score'] for x in r], dtype=np.float64).reshape(n)
        if not np.isfinite(bbox).all() or not np.isfinite(score).all():
            raise ValueError("results: non-finite box or score")
        r = Results(_ids((x['image_id'] for x in r), 'image'), _ids((x['category_id'] for x in r), 'category'), bbox, score)
    if gt is not None:
        gt = load_ground_truth(gt)
        _, ok_i = _index_of(r.image_id, gt.image_ids)
        if not ok_i.all():
            raise ValueError("results name image %d, which the ground truth does not list" % r.image_id[~ok_i][0])
        _, ok_c = _index_of(r.category_id, gt.cat_ids)
        if not ok_c.all():
            r = Results(r.image_id[ok_c], r.category_id[ok_c], r.bbox[ok_c], r.score[ok_c])
    return r


def write_coco_results_file(all_boxes, image_ids, classes, class_to_cat_id, res_file):
    """lib/datasets/coco.py:264-300.  ``all_boxes[cls][img]``: rows [x1, y1, x2, y2, score] (or something empty);
    w = x2 - x1 + 1, h = y2 - y1 + 1; class 0 (the background) is skipped.  Returns the list it wrote."""
    results = []
    for cls_ind, cls in enumerate(classes):
        if cls_ind == 0 or cls == '__background__':
            continue
        cat_id = class_to_cat_id[cls]
        for im_ind, index in enumerate(image_ids):
            dets = np.asarray(all_boxes[cls_ind][im_ind], dtype=np.float64)
            if dets.size == 0:
                continue
            dets = dets.reshape(-1, 5)
            xs, ys = dets[:, 0], dets[:, 1]
            ws, hs = dets[:, 2] - xs + 1, dets[:, 3] - ys + 1
            results.extend({'image_id': int(index), 'category_id': int(cat_id),
                            'bbox': [float(xs[k]), float(ys[k]), float(ws[k]), float(hs[k])], 'score': float(dets[k, 4])}
                           for k in range(dets.shape[0]))
    with open(res_file, 'w') as fid:
        json.dump(results, fid)
    return results


# ----------------------------------------------------------------------------------------------
# prepare: everything up to the matching, on the host, vectorised
# ----------------------------------------------------------------------------------------------
def _group_start(sorted_keys):
    """For keys sorted ascending: the position where each element's run of equal keys begins."""
    n = sorted_keys.shape[0]
    first = np.ones(n, dtype=bool)
    first[1:] = sorted_keys[1:] != sorted_keys[:-1]
    return np.maximum.accumulate(np.where(first, np.arange(n), 0))


def prepare(gt, results, params=None):
    """Pairs in CSR form, in the layout ``frcnn_coco_match`` reads; ordering is decided here.  Returns a dict:
    ``pair_image`` / ``pair_category`` (ids), ``pair_cat_index``, ``det_offsets`` / ``gt_offsets`` / ``iou_offsets``
    (P + 1), ``det`` (D, 5) and ``gt`` (G, 5) float64 [x, y, w, h, area], ``gt_crowd`` (G,) uint8, ``det_scores``,
    ``det_index`` (a kept detection's place among its pair's detections in file order), ``det_rank`` (its place in score
    order), ``cat_ids``."""
    params = params or Params()
    gt = load_ground_truth(gt)
    res = load_results(results, gt)
    K = max(len(gt.cat_ids), 1)
    img_d, _ = _index_of(res.image_id, gt.image_ids)
    cat_d, _ = _index_of(res.category_id, gt.cat_ids)
    key_d = img_d * K + cat_d
    by_key = np.argsort(key_d, kind='stable')
    place = np.empty(len(res), dtype=np.int64)                  # place in file order inside the pair
    place[by_key] = np.arange(len(res)) - _group_start(key_d[by_key])
    order = np.lexsort((-res.score, key_d))                     # by pair, then descending score; lexsort is stable
    rank = np.arange(len(res)) - _group_start(key_d[order])
    keep = order[rank < params.max_dets[-1]]
    key_g = gt.img_index * K + gt.cat_index
    order_g = np.argsort(key_g, kind='stable')                  # annotation order inside a pair
    keys = np.union1d(key_d, key_g)
    p = {'cat_ids': gt.cat_ids, 'pair_image': gt.image_ids[keys // K] if keys.size else np.zeros(0, dtype=np.int64),
         'pair_category': gt.cat_ids[keys % K] if keys.size else np.zeros(0, dtype=np.int64),
         'pair_cat_index': keys % K}
    for name, k in (('det_offsets', key_d[keep]), ('gt_offsets', key_g[order_g])):
        p[name] = np.concatenate([np.searchsorted(k, keys, side='left'), [k.shape[0]]]).astype(np.int64)
    p['iou_offsets'] = np.concatenate([[0], np.cumsum(np.diff(p['det_offsets']) * np.diff(p['gt_offsets']))]).astype(np.int64)
    p['det'] = np.ascontiguousarray(np.concatenate([res.bbox[keep], res.area[keep, None]], axis=1))
    p['gt'] = np.ascontiguousarray(np.concatenate([gt.bbox[order_g], gt.area[order_g, None]], axis=1))
    p['gt_crowd'] = gt.iscrowd[order_g].astype(np.uint8)
    p['det_scores'] = res.score[keep]
    p['det_index'] = place[keep]
    p['det_rank'] = rank[rank < params.max_dets[-1]]
    return p


# ----------------------------------------------------------------------------------------------
# the host path: the protocol as plain loops
# ----------------------------------------------------------------------------------------------
def iou(d, g, crowd):
    """Overlap of detection ``d`` and ground truth ``g``, [x, y, w, h] floats; ``crowd``: the union is the detection's area."""
    dx, dy, dw, dh = d[0], d[1], d[2], d[3]
    gx, gy, gw, gh = g[0], g[1], g[2], g[3]
    iw = min(dx + dw, gx + gw) - max(dx, gx)
    ih = min(dy + dh, gy + gh) - max(dy, gy)
    if iw <= 0 or ih <= 0:
        return 0.0
    i = iw * ih
    u = dw * dh if crowd else dw * dh + gw * gh - i
    return i / u


def match_host(p, params):
    """Overlaps and matching of every pair, literally as the module docstring states them.  Adds to ``p`` what the device
    returns: ``ious`` (flat, pair q's D x G matrix at iou_offsets[q]), ``dt_match`` (D, A, T) int32, ``dt_ignore``
    (D, A, T) bool, ``gt_ignore`` (G, A) bool."""
    A, T = params.area_rng.shape[0], params.iou_thrs.shape[0]
    num_det, num_gt = p['det'].shape[0], p['gt'].shape[0]
    ious = np.zeros(int(p['iou_offsets'][-1]), dtype=np.float64)
    dt_match = np.full((num_det, A, T), -1, dtype=np.int32)
    dt_ignore = np.zeros((num_det, A, T), dtype=bool)
    gt_ignore = np.zeros((num_gt, A), dtype=bool)
    det, gtb, crowd = p['det'].tolist(), p['gt'].tolist(), p['gt_crowd'].astype(bool).tolist()
    thrs, rngs = params.iou_thrs.tolist(), params.area_rng.tolist()
    for q in range(p['det_offsets'].shape[0] - 1):
        d0, d1 = int(p['det_offsets'][q]), int(p['det_offsets'][q + 1])
        g0, g1 = int(p['gt_offsets'][q]), int(p['gt_offsets'][q + 1])
        D, G = d1 - d0, g1 - g0
        ov = [[iou(det[d0 + d], gtb[g0 + g], crowd[g0 + g]) for g in range(G)] for d in range(D)]
        if D and G:
            ious[int(p['iou_offsets'][q]):int(p['iou_offsets'][q + 1])] = np.array(ov, dtype=np.float64).reshape(-1)
        for a, (lo, hi) in enumerate(rngs):
            ig = [crowd[g0 + g] or gtb[g0 + g][4] < lo or gtb[g0 + g][4] > hi for g in range(G)]
            gt_ignore[g0:g1, a] = ig
            visit = sorted(range(G), key=lambda g: ig[g])        # non-ignored first; sorted() is stable
            for t, thr in enumerate(thrs):
                taken = [False] * G
                for d in range(D):
                    best, m = min(thr, 1 - 1e-10), -1
                    for g in visit:
                        if taken[g] and not crowd[g0 + g]:
                            continue
                        if m > -1 and not ig[m] and ig[g]:
                            break
                        if ov[d][g] < best:
                            continue
                        best, m = ov[d][g], g
                    if m > -1:
                        dt_match[d0 + d, a, t] = m
                        dt_ignore[d0 + d, a, t] = ig[m]
                        taken[m] = True
                for d in range(D):
                    if dt_match[d0 + d, a, t] == -1 and (det[d0 + d][4] < lo or det[d0 + d][4] > hi):
                        dt_ignore[d0 + d, a, t] = True
    p.update(ious=ious, dt_match=dt_match, dt_ignore=dt_ignore, gt_ignore=gt_ignore)
    return p


def _empty_tables(p, params):
    T, R, K = params.iou_thrs.shape[0], params.rec_thrs.shape[0], len(p['cat_ids'])
    A, M = params.area_rng.shape[0], len(params.max_dets)
    return -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))


def accumulate_loops(p, params):
    """The accumulate step as plain loops over categories, area ranges, maxDets, thresholds and detections (the host path).
    Returns (precision (T, R, K, A, M), recall (T, K, A, M), scores (T, R, K, A, M))."""
    precision, recall, scores = _empty_tables(p, params)
    T, R = params.iou_thrs.shape[0], params.rec_thrs.shape[0]
    P = p['det_offsets'].shape[0] - 1
    for k in range(len(p['cat_ids'])):
        pairs = [q for q in range(P) if p['pair_cat_index'][q] == k]            # images in order
        for a in range(params.area_rng.shape[0]):
            npig = 0
            for q in pairs:
                for g in range(int(p['gt_offsets'][q]), int(p['gt_offsets'][q + 1])):
                    npig += 0 if p['gt_ignore'][g, a] else 1
            if npig == 0:
                continue
            for mi, M in enumerate(params.max_dets):
                rows = []
                for q in pairs:
                    d0, d1 = int(p['det_offsets'][q]), int(p['det_offsets'][q + 1])
                    rows.extend(range(d0, min(d1, d0 + M)))
                rows = np.array(rows, dtype=np.int64)
                rows = rows[np.argsort(-p['det_scores'][rows], kind='mergesort')]
                sc = p['det_scores'][rows]
                nd = rows.shape[0]
                for t in range(T):
                    tp, fp, rc, pr = 0, 0, [], []
                    for r in rows:
                        matched, ignored = p['dt_match'][r, a, t] >= 0, bool(p['dt_ignore'][r, a, t])
                        tp += 1 if matched and not ignored else 0
                        fp += 1 if not matched and not ignored else 0
                        rc.append(np.float64(tp) / npig)
                        pr.append(np.float64(tp) / (np.float64(fp) + np.float64(tp) + np.spacing(1)))
                    recall[t, k, a, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(np.array(rc, dtype=np.float64), params.rec_thrs, side='left')
                    q_, s_ = np.zeros(R), np.zeros(R)
                    for ri, pi in enumerate(inds):
                        if pi < nd:
                            q_[ri], s_[ri] = pr[pi], sc[pi]
                    precision[t, :, k, a, mi] = q_
                    scores[t, :, k, a, mi] = s_
    return precision, recall, scores


# ----------------------------------------------------------------------------------------------
# the vectorised tail (device path)
# ----------------------------------------------------------------------------------------------
def accumulate(p, params):
    """The accumulate step as vectorised numpy: one stable argsort per (category, maxDet), cumulative sums over all
    thresholds and area ranges at once, the envelope as a reversed np.maximum.accumulate; no Python loop over detections
    or pairs.  Same return as ``accumulate_loops``, equal to it exactly (tests/test_coco_eval_host.py)."""
    precision, recall, scores = _empty_tables(p, params)
    A, T, R = params.area_rng.shape[0], params.iou_thrs.shape[0], params.rec_thrs.shape[0]
    K = len(p['cat_ids'])
    pair_of_det = np.repeat(np.arange(p['det_offsets'].shape[0] - 1), np.diff(p['det_offsets']))
    pair_of_gt = np.repeat(np.arange(p['gt_offsets'].shape[0] - 1), np.diff(p['gt_offsets']))
    cat_of_det, cat_of_gt = p['pair_cat_index'][pair_of_det], p['pair_cat_index'][pair_of_gt]
    npig = np.zeros((K, A), dtype=np.int64)
    np.add.at(npig, cat_of_gt, ~p['gt_ignore'].astype(bool))
    by_cat = np.argsort(cat_of_det, kind='stable')              # per category: images in order, score order inside a pair
    bounds = np.searchsorted(cat_of_det[by_cat], np.arange(K + 1), side='left')
    matched_all, ignored_all = p['dt_match'] >= 0, p['dt_ignore'].astype(bool)
    for k in range(K):
        if not npig[k].any():
            continue
        dets_k = by_cat[bounds[k]:bounds[k + 1]]
        live = npig[k] > 0                                      # area ranges with non-ignored ground truth
        for mi, M in enumerate(params.max_dets):
            rows = dets_k[p['det_rank'][dets_k] < M]
            rows = rows[np.argsort(-p['det_scores'][rows], kind='mergesort')]
            nd = rows.shape[0]
            sc = p['det_scores'][rows]
            matched, ignored = matched_all[rows], ignored_all[rows]                      # (nd, A, T)
            tp = np.cumsum(matched & ~ignored, axis=0).astype(np.float64)
            fp = np.cumsum(~matched & ~ignored, axis=0).astype(np.float64)
            rc = tp / np.maximum(npig[k], 1)[None, :, None]
            pr = tp / (fp + tp + np.spacing(1))
            pr = np.maximum.accumulate(pr[::-1], axis=0)[::-1]
            rec_k = rc[-1] if nd else np.zeros((A, T))
            recall[:, k, live, mi] = rec_k[live].T
            q_, s_ = np.zeros((R, A, T)), np.zeros((R, A, T))
            for a in np.nonzero(live)[0]:
                for t in range(T):
                    inds = np.searchsorted(rc[:, a, t], params.rec_thrs, side='left')
                    ok = inds < nd
                    q_[ok, a, t] = pr[inds[ok], a, t]
                    s_[ok, a, t] = sc[inds[ok]]
            precision[:, :, k, live, mi] = q_[:, live, :].transpose(2, 0, 1)
            scores[:, :, k, live, mi] = s_[:, live, :].transpose(2, 0, 1)
    return precision, recall, scores


# ----------------------------------------------------------------------------------------------
# summary
# ----------------------------------------------------------------------------------------------
def _mean_valid(s):
    s = s[s > -1]
    return float(np.mean(s)) if s.size else -1.0


def _stat_specs(params):
    """(is AP, IoU threshold or None, area label, maxDet) of the 12 summary numbers, in the published order."""
    md = params.max_dets
    last = md[-1]
    return [(True, None, 'all', last), (True, .5, 'all', last), (True, .75, 'all', last),
            (True, None, 'small', last), (True, None, 'medium', last), (True, None, 'large', last),
            (False, None, 'all', md[0]), (False, None, 'all', md[min(1, len(md) - 1)]), (False, None, 'all', md[min(2, len(md) - 1)]),
            (False, None, 'small', last), (False, None, 'medium', last), (False, None, 'large', last)]


def _stat(precision, recall, params, is_ap, iou_thr, area, max_det):
    if area not in params.area_lbl:
        return -1.0
    a, m = params.area_lbl.index(area), params.max_dets.index(max_det)
    s = precision[:, :, :, a, m] if is_ap else recall[:, :, a, m]
    if iou_thr is not None:
        t = np.nonzero(np.isclose(params.iou_thrs, iou_thr, rtol=0, atol=1e-9))[0]
        if not t.size:
            return -1.0
        s = s[t]
    return _mean_valid(s)


def compute_stats(precision, recall, params):
    """The 12 summary numbers: AP, AP50, AP75, AP small / medium / large, AR@1 / @10 / @100, AR small / medium / large;
    each the mean over entries > -1, and -1 if there are none (or the parameters have no such threshold / area label)."""
    return np.array([_stat(precision, recall, params, *spec) for spec in _stat_specs(params)], dtype=np.float64)


def summarize(result):
    """The 12 lines in the published format."""
    params = result['params']
    lines = []
    for spec, value in zip(_stat_specs(params), result['stats']):
        is_ap, iou_thr, area, max_det = spec
        iou_str = ('{:0.2f}:{:0.2f}'.format(params.iou_thrs[0], params.iou_thrs[-1]) if iou_thr is None
                   else '{:0.2f}'.format(iou_thr))
        lines.append(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
            'Average Precision' if is_ap else 'Average Recall', '(AP)' if is_ap else '(AR)', iou_str, area, max_det, value))
    return lines


def print_detection_eval_metrics(result, classes):
    """What lib/datasets/coco.py:217-249 prints: the mean AP@[.50:.95] at area 'all' and the largest maxDets overall, then
    per foreground class (category k belongs to classes[k + 1]), '{:.1f}' of 100 x, then the summary.  Returns the lines."""
    params = result['params']
    lo = np.nonzero((params.iou_thrs > .5 - 1e-5) & (params.iou_thrs < .5 + 1e-5))[0][0]
    hi = np.nonzero((params.iou_thrs > .95 - 1e-5) & (params.iou_thrs < .95 + 1e-5))[0][0]
    m = len(params.max_dets) - 1
    block = result['precision'][lo:hi + 1, :, :, 0, m]
    lines = ['~~~~ Mean and per-category AP @ IoU=[{:.2f},{:.2f}] ~~~~'.format(.5, .95),
             '{:.1f}'.format(100 * _mean_valid(block))]
    for cls_ind, cls in enumerate(classes):
        if cls_ind == 0 or cls == '__background__':
            continue
        lines.append('{:.1f}'.format(100 * _mean_valid(block[:, :, cls_ind - 1])))
    lines.append('~~~~ Summary metrics ~~~~')
    lines.extend(summarize(result))
    for line in lines:
        print(line)
    return lines


# ----------------------------------------------------------------------------------------------
# evaluate
# ----------------------------------------------------------------------------------------------
def match_device(p, params, device='cuda'):
    """Upload, one ``frcnn_coco_match`` launch, read back: what ``match_host`` adds to ``p``, from the device."""
    import torch
    from .. import ops

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    ious, _, dt_match, dt_ignore, gt_ignore = ops.coco_match(
        up(p['det']), p['det_offsets'], up(p['gt']), up(p['gt_crowd']), p['gt_offsets'], params.iou_thrs, params.area_rng)
    dt_match = dt_match.cpu().numpy()
    if (dt_match < -1).any():
        raise RuntimeError("frcnn_coco_match left a pair unscored")
    p.update(ious=ious.cpu().numpy(), dt_match=dt_match, dt_ignore=dt_ignore.cpu().numpy().astype(bool),
             gt_ignore=gt_ignore.cpu().numpy().astype(bool))
    return p


def evaluate(gt, results, params=None, device=None):
    """Score a results list against the ground truth.  ``gt``: a ``GroundTruth``, an annotation dict or a file; ``results``:
    a ``Results``, a results list or a file.  Returns a dict: ``precision`` (T, R, K, A, M) and ``scores`` of the same shape,
    ``recall`` (T, K, A, M) (-1 where a category has no non-ignored ground truth), ``stats`` (the 12 summary numbers),
    ``params``, and the per-pair matches - everything ``prepare`` returns plus ``ious``, ``dt_match`` (D, A, T; the matched
    box inside the pair in annotation order, or -1), ``dt_ignore`` and ``gt_ignore`` (G, A).
    ``device=None``: the host path (plain loops); ``device='cuda'`` (or any torch device string): matching by one
    ``frcnn_coco_match`` launch, vectorised tail."""
    params = params or Params()
    p = prepare(gt, results, params)
    if device is None:
        match_host(p, params)
        precision, recall, scores = accumulate_loops(p, params)
    else:
        match_device(p, params, device)
        precision, recall, scores = accumulate(p, params)
    p.update(precision=precision, recall=recall, scores=scores, params=params,
             stats=compute_stats(precision, recall, params))
    return p


def evaluate_detections(all_boxes, image_ids, classes, class_to_cat_id, gt, output_dir, device=None):
    """lib/datasets/coco.py:302-312 without salt and cleanup: write ``detections_results.json`` under ``output_dir``,
    evaluate, print the metrics and pickle the result dict to ``detection_results.pkl``.  Returns the result dict."""
    res_file = os.path.join(output_dir, 'detections_results.json')
    write_coco_results_file(all_boxes, image_ids, classes, class_to_cat_id, res_file)
    result = evaluate(gt, res_file, device=device)
    print_detection_eval_metrics(result, classes)
    eval_file = os.path.join(output_dir, RESULTS_PICKLE)
    with open(eval_file, 'wb') as fid:
        pickle.dump(result, fid, pickle.HIGHEST_PROTOCOL)
    print('Wrote COCO eval results to: {}'.format(eval_file))
    return result
