"""The evaluators' overlap-and-match loop on the device (``frcnn_eval_match``, csrc/eval_match.hip), shared by
``waymo_eval`` / ``kitti_eval`` / ``cadc_eval`` when they are called with ``device='cuda'`` - counterpart of
lib/datasets/waymo_eval.py:131-213, kitti_eval.py:116-215 and cadc_eval.py:115-206 (one loop, three copies).

Host side (``prepare``): what the loop does per detection before it computes an overlap, done once for the file -
  * ``find_rec`` as ONE dict: a token names the FIRST record with that filename whose ``ignore_frame`` is false;
  * detections without a record are dropped without consuming a row of the tp / fp tables;
  * the rest are visited in the order of ``np.argsort(-confidence)`` (numpy's tie order: it is an INPUT of the device,
    which never sorts) - a detection's place in that order is its ROW;
  * detections, ground truth and don't-care boxes are grouped by frame (CSR), rows ascending inside a frame.
Device side: overlaps, first-maximum, don't-care maximum and the matching, all frames in one launch.
Tail (``ap_tail``): the evaluators' cumulative sums, ``sorted(zip(rec, prec))`` and AP as vectorised numpy.

PARITY UNPINNED against shapely / the reference's missing ``eval_utils``; equal to this package's float64 host path
(``waymo_eval.iou`` and the host loops): tests/test_eval_device.py.
"""
import numpy as np

from .waymo_eval import ap

EVAL_ELEMS = {'2d': 4, 'bev_aa': 7, 'bev': 7, '3d': 7}


class Prepared(object):
    """The file's detections and the records' boxes in the layout the kernel reads.  ``row_of_det[i]``: row of detection
    i of the file, -1 when it has no record; ``rec_of_frame[f]``: index in class_recs of frame f; ``frame_of_row[r]``;
    ``slot_of_row[r]``: where row r sits in the frame-grouped arrays (``det_rows[slot_of_row[r]] == r``)."""
    __slots__ = ('eval_type', 'row_of_det', 'rec_of_frame', 'frame_of_row', 'slot_of_row', 'det_boxes', 'det_rows',
                 'det_offsets', 'gt_boxes', 'gt_ignore', 'gt_difficulty', 'gt_offsets', 'dc_boxes', 'dc_offsets',
                 'max_gt_per_frame')


def token_map(class_recs):
    """{filename: index of the first record with that filename that is not ``ignore_frame``}: ``find_rec`` for every
    token at once (a later duplicate of a filename is never reached by the linear scan either)."""
    first = {}
    for i, rec in enumerate(class_recs):
        name = rec.get('filename')
        if name not in first and not rec.get('ignore_frame', False):
            first[name] = i
    return first


def _check_boxes(boxes, what, eval_type):
    if boxes.size and not np.isfinite(boxes).all():
        raise ValueError("%s: non-finite box value" % what)
    if eval_type != '2d' and boxes.size and (boxes[:, 3:6] <= 0).any():
        raise ValueError("%s: l, w and h must be > 0 for eval_type %r" % (what, eval_type))


def _stack(per_frame, elem):
    counts = np.array([b.shape[0] for b in per_frame], dtype=np.int64)
    offsets = np.zeros(len(per_frame) + 1, dtype=np.int32)
    np.cumsum(counts, out=offsets[1:])
    rows = [b for b in per_frame if b.shape[0]]
    return (np.concatenate(rows, axis=0) if rows else np.zeros((0, elem))), offsets


def prepare(frame_tokens, confidence, boxes, class_recs, eval_type, ignore_dc):
    """Everything up to the launch, on the host (no device needed).  Raises ValueError for an unknown ``eval_type``, for a
    non-finite box value and, with a 'bev' / 'bev_aa' / '3d' type, for l, w or h <= 0 (where the host path divides 0 by
    0) - checked on the detections that have a record and on the boxes of the records that detections can name."""
    if eval_type not in EVAL_ELEMS:
        raise ValueError("eval_type %r" % (eval_type,))
    elem = EVAL_ELEMS[eval_type]
    confidence = np.asarray(confidence, dtype=np.float64).reshape(-1)
    n = confidence.shape[0]
    boxes = np.asarray(boxes, dtype=np.float64)
    boxes = boxes.reshape(n, -1) if n else np.zeros((0, elem))
    if len(frame_tokens) != n:
        raise ValueError("%d tokens for %d confidences" % (len(frame_tokens), n))
    if n and boxes.shape[1] < elem:
        raise ValueError("eval_type %r needs %d box elements, got %d" % (eval_type, elem, boxes.shape[1]))
    first = token_map(class_recs)
    rec_of_frame = np.array(sorted(first.values()), dtype=np.int64)
    frame_of_rec = {int(r): f for f, r in enumerate(rec_of_frame)}
    rec_of_det = np.array([first.get(t, -1) for t in frame_tokens], dtype=np.int64)
    order = np.argsort(-confidence) if n else np.zeros(0, dtype=np.int64)      # the reference's very call
    kept = order[rec_of_det[order] >= 0]
    p = Prepared()
    p.eval_type = eval_type
    p.row_of_det = np.full(n, -1, dtype=np.int64)
    p.row_of_det[kept] = np.arange(kept.shape[0])
    p.rec_of_frame = rec_of_frame
    p.frame_of_row = np.array([frame_of_rec[int(r)] for r in rec_of_det[kept]], dtype=np.int64)
    by_frame = np.argsort(p.frame_of_row, kind='stable')                        # rows ascending inside a frame
    p.slot_of_row = np.empty(kept.shape[0], dtype=np.int64)
    p.slot_of_row[by_frame] = np.arange(kept.shape[0])
    p.det_rows = by_frame.astype(np.int32)
    p.det_boxes = np.ascontiguousarray(boxes[kept][by_frame][:, :elem]) if kept.shape[0] else np.zeros((0, elem))
    p.det_offsets = np.zeros(rec_of_frame.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(p.frame_of_row, minlength=rec_of_frame.shape[0]), out=p.det_offsets[1:])
    _check_boxes(p.det_boxes, "detections", eval_type)

    def of(rec, key):
        b = np.asarray(rec[key], dtype=np.float64)
        return b.reshape(b.shape[0], -1)[:, :elem] if b.size else np.zeros((0, elem))

    recs = [class_recs[int(r)] for r in rec_of_frame]
    p.gt_boxes, p.gt_offsets = _stack([of(rec, 'boxes') for rec in recs], elem)
    counts = np.diff(p.gt_offsets)
    for rec, c in zip(recs, counts):
        if c and (len(rec['ignore']) != c or len(rec['difficulty']) != c):
            raise ValueError("record %r: %d boxes, %d ignore flags, %d difficulties"
                             % (rec.get('filename'), c, len(rec['ignore']), len(rec['difficulty'])))
    p.gt_ignore = np.concatenate([np.asarray(rec['ignore'], dtype=bool) for rec, c in zip(recs, counts) if c]
                                 or [np.zeros(0, dtype=bool)]).astype(np.uint8)
    p.gt_difficulty = np.concatenate([np.asarray(rec['difficulty'], dtype=np.int64) for rec, c in zip(recs, counts) if c]
                                     or [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    p.max_gt_per_frame = int(counts.max()) if counts.size else 0
    _check_boxes(p.gt_boxes, "ground truth", eval_type)
    p.dc_boxes = p.dc_offsets = None
    if ignore_dc:
        p.dc_boxes, p.dc_offsets = _stack([of(rec, 'boxes_dc') for rec in recs], elem)
        _check_boxes(p.dc_boxes, "don't-care boxes", eval_type)
    return p


def match(frame_tokens, confidence, boxes, class_recs, ovthresh, eval_type, ignore_dc, ovthresh_dc=0.5, device='cuda'):
    """``prepare``, upload, one ``frcnn_eval_match`` launch, read back.  Returns a dict of arrays: ``row_of_det`` per
    detection of the file and, per row, ``code`` (ops.EVAL_NONE / EVAL_TP / EVAL_DUP_FP / EVAL_FP), ``jmax``, ``ovmax``,
    ``ovmax_dc``, ``difficulty`` (of the matched box for EVAL_TP / EVAL_DUP_FP, else -1) and ``rec`` (index in
    class_recs of the row's frame).  Every record's ``hit`` is left as the host loop leaves it."""
    import torch
    from .. import ops
    p = prepare(frame_tokens, confidence, boxes, class_recs, eval_type, ignore_dc)
    for rec in class_recs:
        if 'hit' in rec:
            rec['hit'][:] = False
    rows = p.det_rows.shape[0]
    out = {'row_of_det': p.row_of_det, 'rec': p.rec_of_frame[p.frame_of_row] if rows else np.zeros(0, dtype=np.int64)}
    if p.rec_of_frame.shape[0] == 0:
        empty = np.zeros(0)
        out.update(code=empty.astype(np.int32), jmax=empty.astype(np.int32), ovmax=empty, ovmax_dc=empty.copy(),
                   difficulty=empty.astype(np.int32))
        return out

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    code, jmax, ovmax, ovmax_dc, dif, hit = ops.eval_match(
        up(p.det_boxes), up(p.det_rows), up(p.det_offsets), up(p.gt_boxes), up(p.gt_ignore), up(p.gt_difficulty),
        up(p.gt_offsets), eval_type, ovthresh, ovthresh_dc, None if p.dc_boxes is None else up(p.dc_boxes),
        None if p.dc_offsets is None else up(p.dc_offsets), max_gt_per_frame=p.max_gt_per_frame)
    s = p.slot_of_row
    out.update(code=code.cpu().numpy()[s], jmax=jmax.cpu().numpy()[s], ovmax=ovmax.cpu().numpy()[s],
               ovmax_dc=ovmax_dc.cpu().numpy()[s], difficulty=dif.cpu().numpy()[s])
    if (out['code'] < 0).any():
        raise RuntimeError("frcnn_eval_match left a frame unscored")
    hit = hit.cpu().numpy().astype(bool)
    for f, r in enumerate(p.rec_of_frame):
        rec = class_recs[int(r)]
        if 'hit' in rec and p.gt_offsets[f + 1] > p.gt_offsets[f]:
            rec['hit'][:] = hit[p.gt_offsets[f]:p.gt_offsets[f + 1]]
    return out


def match_detections(frame_tokens, confidence, boxes, class_recs, ovthresh, eval_type, ignore_dc, device='cuda'):
    """The matching loop of the three evaluators on the device.  ``frame_tokens`` / ``confidence`` / ``boxes``: one entry
    per line of the detections file; ``class_recs``: the per-frame records (``waymo_eval.make_rec``).
    Returns ``(row_of_det, code, jmax, ovmax, ovmax_dc)`` as numpy arrays: the row of each detection in the tp / fp
    tables (-1: its token has no record, no row consumed) and, per row, the verdict code, the index of the best ground
    truth box inside its frame, its overlap and the largest don't-care overlap.  ``rec['hit']`` of every record is
    written exactly as the host loop leaves it.
    Raises ValueError when a box value is not finite and, for 'bev' / 'bev_aa' / '3d', when l, w or h is <= 0 (the
    host path divides 0 by 0 there)."""
    m = match(frame_tokens, confidence, boxes, class_recs, ovthresh, eval_type, ignore_dc, device=device)
    return m['row_of_det'], m['code'], m['jmax'], m['ovmax'], m['ovmax_dc']


def scatter_tables(n, d_levels, m, level_offset):
    """tp / fp tables (n, d_levels) from the verdict codes: a true positive / duplicate counts at the levels with
    ``difficulty <= lvl + level_offset`` (waymo: 1; kitti, cadc: 0, columns 0..2 only), a plain false positive at all."""
    from ..ops import EVAL_DUP_FP, EVAL_FP, EVAL_TP
    tp, fp = np.zeros((n, d_levels)), np.zeros((n, d_levels))
    rows = m['code'].shape[0]
    cols = d_levels if level_offset else min(d_levels, 3)
    if rows:
        at_level = m['difficulty'][:, None] <= (np.arange(cols) + level_offset)[None, :]
        tp[:rows, :cols] += at_level & (m['code'] == EVAL_TP)[:, None]
        fp[:rows, :cols] += at_level & (m['code'] == EVAL_DUP_FP)[:, None]
        fp[:rows, :cols] += (m['code'] == EVAL_FP)[:, None]
    return tp, fp


def ap_tail(tp, fp, npos, d_levels):
    """The evaluators' tail (waymo_eval.py:232-247) without Python loops over detections: cumulative sums, the
    lexicographic sort of the (rec, prec) PAIRS, their un-aliased means and the VOC envelope.  Returns
    (ap, mean_recall, mean_precision), each (d_levels,)."""
    ap_d, mrec, mprec = np.zeros(d_levels), np.zeros(d_levels), np.zeros(d_levels)
    fp_sum, tp_sum, npos_sum = np.cumsum(fp, axis=0), np.cumsum(tp, axis=0), np.sum(npos, axis=0)
    for i in range(d_levels):
        npos_d = npos_sum[i] if npos_sum[i] != 0 else 1.0
        rec_c = tp_sum[:, i] / float(npos_d)
        prec_c = tp_sum[:, i] / np.maximum(tp_sum[:, i] + fp_sum[:, i], np.finfo(np.float64).eps)
        order = np.lexsort((prec_c, rec_c))              # sorted(zip(rec, prec)): by rec, ties by prec
        rec_c, prec_c = rec_c[order], prec_c[order]
        mprec[i] = np.average(prec_c) if len(prec_c) else 0.0
        mrec[i] = np.average(rec_c) if len(rec_c) else 0.0
        ap_d[i] = ap(rec_c, prec_c)
    return ap_d, mrec, mprec


def evaluate_on_device(frame_tokens, confidence, boxes, class_recs, ovthresh, eval_type, ignore_dc, d_levels, npos,
                       level_offset, device):
    """The ``device=`` branch of the three evaluators: matching from the device, tables from the codes, the vectorised
    tail.  Returns what they return: three views of ONE array that holds the AP per level (``map = mrec = mprec``,
    waymo_eval.py:232) and the dict of un-aliased quantities, which here also carries ``jmax`` / ``ovmax`` / ``code`` per
    row (what the reference's ``write_det`` prints; the caller formats the lines)."""
    m = match(frame_tokens, confidence, boxes, class_recs, ovthresh, eval_type, ignore_dc, device=device)
    tp, fp = scatter_tables(len(frame_tokens), d_levels, m, level_offset)
    ap_d, mrec, mprec = ap_tail(tp, fp, npos, d_levels)
    shared = ap_d.copy()
    plain = {'ap': ap_d, 'mean_recall': mrec, 'mean_precision': mprec, 'tp': tp, 'fp': fp, 'npos': npos,
             'jmax': m['jmax'], 'ovmax': m['ovmax'], 'code': m['code']}
    return shared, shared, shared, plain
