"""KITTI-style scoring of a detections file - counterpart of lib/datasets/kitti_eval.py:44-282 (kitti_eval, count_npos).

The loop is the one of ``waymo_eval`` (datasets/waymo_eval.py, whose module docstring lists what is restated and what
is not: ``find_rec`` / ``iou`` / ``ap`` come from there); what differs is the difficulty rule:
  * a box counts at level ``lvl`` (0 easy, 1 moderate, 2 hard) when ``difficulty <= lvl`` (:179-184,192-197,276-281);
  * the reference indexes columns 0, 1 and 2 unconditionally, so ``d_levels`` must be 3: anything else raises ValueError
    (the reference would raise IndexError below 3 and leave extra columns untouched above).
Kept from the reference: ``map = mrec = mprec = np.zeros(...)`` aliases ONE array, so the three returned arrays hold the
AP; the un-aliased means are returned in the dict.  Not restated: annotation loading (``load_recs``, including its
"difficulty outside {0, 1, 2} -> ignore" rule: the caller's job, as for ``waymo_eval``), the per-frame counters and the
``write_det`` text lines (the dict of the device branch carries what they print).  An empty detections file, where the
reference fails on ``zip(*sorted(...))``, gives zeros.

PARITY UNPINNED against shapely / the reference's missing ``eval_utils``; ``device='cuda'`` equals this module's host
loop (tests/test_eval_device.py).
"""
import numpy as np

from ..model.config import cfg
from .waymo_eval import ap, find_rec, iou


def count_npos(class_recs, d_levels):
    """kitti_eval.py:271-282: non-ignored boxes of non-ignored frames, per level."""
    npos = np.zeros((len(class_recs), d_levels))
    for i, rec in enumerate(class_recs):
        if rec.get('ignore_frame') is False:
            for j, ig in enumerate(rec['ignore']):
                if not ig:
                    for lvl in range(min(d_levels, 3)):
                        if rec['difficulty'][j] <= lvl:
                            npos[i, lvl] += 1
    return npos


def kitti_eval(detfile, class_recs, ovthresh=0.5, eval_type='2d', d_levels=3, bbox_elem=None, ignore_dc=None, device=None):
    """Returns (mrec, mprec, map) as the reference does (three views of ONE array holding the AP per difficulty level)
    plus a dict with the un-aliased quantities: {'ap', 'mean_recall', 'mean_precision', 'tp', 'fp', 'npos'}.
    ``device='cuda'``: overlaps and matching from one ``frcnn_eval_match`` launch, vectorised tail
    (datasets/device_eval.py); same results, and the dict also carries 'jmax', 'ovmax' and 'code' per row.
    ``d_levels`` must be 3 (ValueError otherwise)."""
    if d_levels != 3:
        raise ValueError("kitti_eval indexes difficulty columns 0, 1 and 2: d_levels must be 3, got %r" % (d_levels,))
    ovthresh_dc = 0.5
    bbox_elem = bbox_elem if bbox_elem is not None else cfg[cfg.NET_TYPE.upper()].NUM_BBOX_ELEM
    ignore_dc = bool(cfg.TEST.get('IGNORE_DC', False)) if ignore_dc is None else ignore_dc
    with open(detfile, 'r') as f:
        splitlines = [x.strip().split(' ') for x in f.readlines() if x.strip()]
    frame_tokens = [x[1] for x in splitlines]
    confidence = np.array([float(x[2]) for x in splitlines])
    bb_all = np.array([[float(z) for z in x[3:3 + bbox_elem]] for x in splitlines]).reshape(len(splitlines), bbox_elem)
    n = len(splitlines)
    tp, fp = np.zeros((n, d_levels)), np.zeros((n, d_levels))
    npos = count_npos(class_recs, d_levels)
    if device is not None:
        from .device_eval import evaluate_on_device
        return evaluate_on_device(frame_tokens, confidence, bb_all, class_recs, ovthresh, eval_type, ignore_dc, d_levels,
                                  npos, 0, device)
    for rec in class_recs:
        if 'hit' in rec:
            rec['hit'][:] = False
    idx = 0
    if bb_all.shape[0] > 0:
        for det_idx in np.argsort(-confidence):                              # :118-130
            rec = find_rec(class_recs, frame_tokens[det_idx])
            if rec is None:
                continue
            bb = bb_all[det_idx, :].astype(float)
            ovmax, jmax = -np.inf, 0
            bbgt, bbgt_dc = rec['boxes'].astype(float), rec['boxes_dc'].astype(float)
            ovmax_dc = 0
            if bbgt_dc.size > 0 and ignore_dc:
                ovmax_dc = np.max(iou(bbgt_dc, bb, eval_type))
            if bbgt.size > 0:
                overlaps = iou(bbgt, bb, eval_type)
                ovmax, jmax = np.max(overlaps), int(np.argmax(overlaps))
            if ovmax > ovthresh and ovmax_dc < ovthresh_dc:                  # :173-199
                if not rec['ignore'][jmax]:
                    table = fp if rec['hit'][jmax] else tp
                    if rec['difficulty'][jmax] <= 2:
                        table[idx, 2] += 1
                    if rec['difficulty'][jmax] <= 1:
                        table[idx, 1] += 1
                    if rec['difficulty'][jmax] <= 0:
                        table[idx, 0] += 1
                    rec['hit'][jmax] = True
            elif bbgt.size > 0 and ovmax_dc < ovthresh_dc:                   # :201-214
                fp[idx, 2] += 1
                fp[idx, 1] += 1
                fp[idx, 0] += 1
            idx += 1
    shared = np.zeros((d_levels,))                                            # map = mrec = mprec
    plain = {'ap': np.zeros(d_levels), 'mean_recall': np.zeros(d_levels), 'mean_precision': np.zeros(d_levels),
             'tp': tp, 'fp': fp, 'npos': npos}
    fp_sum, tp_sum, npos_sum = np.cumsum(fp, axis=0), np.cumsum(tp, axis=0), np.sum(npos, axis=0)
    for i in range(d_levels):
        npos_d = npos_sum[i] if npos_sum[i] != 0 else 1.0
        rec_c = tp_sum[:, i] / float(npos_d)
        prec_c = tp_sum[:, i] / np.maximum(tp_sum[:, i] + fp_sum[:, i], np.finfo(np.float64).eps)
        if len(rec_c):
            rec_c, prec_c = zip(*sorted(zip(rec_c, prec_c)))
        plain['mean_precision'][i] = np.average(prec_c) if len(prec_c) else 0.0
        plain['mean_recall'][i] = np.average(rec_c) if len(rec_c) else 0.0
        plain['ap'][i] = ap(rec_c, prec_c)
        shared[i] = plain['ap'][i]
    return shared, shared, shared, plain
