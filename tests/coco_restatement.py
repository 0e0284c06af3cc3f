"""A second statement of the COCO protocol's *accumulate* and *summarize* steps, written for the tests as plain loops over
per-image records, independently of the package's tails (datasets/coco_eval.py ``accumulate`` and ``accumulate_loops``).
It reads only the per-pair matches of a result dict: offsets, scores, ``dt_match``, ``dt_ignore``, ``gt_ignore``."""
import numpy as np


def per_image_records(r):
    """{category index: [record per pair, images in order]}; a record holds the pair's scores and, per (a, t), the
    detections' matched and ignore flags as Python lists, and per a the ground truth's ignore flags."""
    recs = {}
    for q in range(len(r['pair_cat_index'])):
        d0, d1 = int(r['det_offsets'][q]), int(r['det_offsets'][q + 1])
        g0, g1 = int(r['gt_offsets'][q]), int(r['gt_offsets'][q + 1])
        recs.setdefault(int(r['pair_cat_index'][q]), []).append({
            'scores': [float(s) for s in r['det_scores'][d0:d1]],
            'matched': (np.asarray(r['dt_match'][d0:d1]) >= 0),
            'dt_ignore': np.asarray(r['dt_ignore'][d0:d1]).astype(bool),
            'gt_ignore': np.asarray(r['gt_ignore'][g0:g1]).astype(bool)})
    return recs


def accumulate(r, params):
    T, R, K = len(params.iou_thrs), len(params.rec_thrs), len(r['cat_ids'])
    A, M = len(params.area_rng), len(params.max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    recs = per_image_records(r)
    for k in range(K):
        for a in range(A):
            for mi, max_det in enumerate(params.max_dets):
                images = recs.get(k, [])
                npig = sum(int(not flag) for e in images for flag in e['gt_ignore'][:, a])
                if npig == 0:
                    continue
                entries = []                                    # (score, position, image record, detection)
                for e in images:
                    for d in range(min(max_det, len(e['scores']))):
                        entries.append((e['scores'][d], len(entries), e, d))
                entries.sort(key=lambda x: (-x[0], x[1]))       # descending score, ties in concatenation order
                for t in range(T):
                    tp = fp = 0
                    rc, pr = [], []
                    for s, _, e, d in entries:
                        if not e['dt_ignore'][d, a, t]:
                            if e['matched'][d, a, t]:
                                tp += 1
                            else:
                                fp += 1
                        rc.append(tp / npig)
                        pr.append(tp / (fp + tp + np.spacing(1)))
                    recall[t, k, a, mi] = rc[-1] if entries else 0
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, thr in enumerate(params.rec_thrs):
                        i = 0
                        while i < len(rc) and rc[i] < thr:      # searchsorted, side='left'
                            i += 1
                        precision[t, ri, k, a, mi] = pr[i] if i < len(rc) else 0
                        scores[t, ri, k, a, mi] = entries[i][0] if i < len(rc) else 0
    return precision, recall, scores


def _mean(values):
    values = [v for v in np.asarray(values).reshape(-1) if v > -1]
    return float(np.mean(values)) if values else -1.0


def stats(precision, recall, params):
    """The 12 summary numbers for the DEFAULT labels (all / small / medium / large) and three maxDets."""
    lbl = list(params.area_lbl)
    last = len(params.max_dets) - 1

    def ap(a, thr=None):
        if thr is None:
            return _mean(precision[:, :, :, lbl.index(a), last])
        t = [i for i, v in enumerate(params.iou_thrs) if abs(v - thr) < 1e-9]
        return _mean(precision[t[0], :, :, lbl.index(a), last]) if t else -1.0

    def ar(a, m):
        return _mean(recall[:, :, lbl.index(a), m])

    return np.array([ap('all'), ap('all', .5), ap('all', .75), ap('small'), ap('medium'), ap('large'),
                     ar('all', 0), ar('all', 1), ar('all', 2), ar('small', last), ar('medium', last), ar('large', last)])
