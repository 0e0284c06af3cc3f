"""Seeded scenes and the recording host walk shared by tests/test_eval_hosts.py and tests/test_eval_device.py.

``host_walk`` is the evaluators' loop (datasets/waymo_eval.py: ``find_rec`` per detection, ``iou``, the sequential
``hit`` walk) with every intermediate value kept: per row the verdict code, jmax, ovmax, ovmax_dc and all overlaps.
It calls the package's own ``find_rec`` and ``iou`` (the float64 host path) and nothing of the device path."""
import functools

import numpy as np

from faster_rcnn_pytorch_multimodal_amd.datasets import waymo_eval as Wm

NONE, TP, DUP_FP, FP = 0, 1, 2, 3
# per-frame gt counts straddling the kernel's LDS chunk (FRCNN_EVAL_CHUNK = 64)
GT_COUNTS = (0, 1, 5, 63, 64, 65, 3, 17)


def random_boxes(rng, n):
    return np.column_stack((rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-1, 1, n), rng.uniform(3, 5, n),
                            rng.uniform(1.5, 2.5, n), rng.uniform(1.4, 2.0, n), rng.uniform(-np.pi, np.pi, n)))


def jitter(rng, boxes):
    out = boxes.copy()
    n = len(boxes)
    out[:, :3] += rng.normal(0, 0.3, (n, 3))
    out[:, 3:6] *= rng.uniform(0.9, 1.1, (n, 3))
    out[:, 6] += rng.normal(0, 0.1, n)
    return out


def to_2d(boxes):
    """[xc,yc,zc,l,w,h,ry] -> pixel boxes [x1,y1,x2,y2] (10 px per metre), for the '2d' type."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    return np.column_stack((b[:, 0] - b[:, 3] / 2, b[:, 1] - b[:, 4] / 2, b[:, 0] + b[:, 3] / 2, b[:, 1] + b[:, 4] / 2)) * 10 + 400


@functools.lru_cache(maxsize=None)
def _scene(seed, gt_counts, two_d):
    rng = np.random.default_rng(seed)
    recs, tokens, conf, boxes = [], [], [], []
    for f, ng in enumerate(gt_counts):
        name = "%06d.bin" % f
        gt = random_boxes(rng, ng)
        dc = random_boxes(rng, int(rng.integers(0, 4)))
        det = [jitter(rng, gt), jitter(rng, gt[rng.random(ng) < 0.5]), random_boxes(rng, int(rng.integers(0, 6))),
               jitter(rng, dc)]
        det = np.concatenate(det, axis=0)
        if two_d:
            gt, dc, det = to_2d(gt), to_2d(dc), to_2d(det)
        recs.append(Wm.make_rec(name, gt if ng else np.zeros((0, gt.shape[1])), difficulty=rng.integers(0, 4, ng),
                                ignore=rng.random(ng) < 0.15, boxes_dc=dc.reshape(-1, gt.shape[1]), ignore_frame=False))
        tokens += [name] * len(det)
        conf += list(rng.uniform(0.05, 1.0, len(det)))
        boxes.append(det)
    return recs, tokens, np.array(conf), np.concatenate(boxes, axis=0)


def scene(seed, gt_counts=GT_COUNTS, eval_type='bev'):
    """(class_recs, frame_tokens, confidence, boxes): jittered copies of the gt boxes (centre sigma 0.3 m, dimensions x
    U(0.9, 1.1), yaw sigma 0.1), second copies of about half of them, 0-5 random boxes per frame and a jittered copy of
    every don't-care box; random ``ignore``, difficulties in {0, 1, 2, 3}, 0-3 don't-care boxes per frame.  The records
    are fresh copies (``hit`` is written by the evaluators)."""
    recs, tokens, conf, boxes = _scene(seed, tuple(gt_counts), eval_type == '2d')
    return [dict(r, hit=r['hit'].copy()) for r in recs], list(tokens), conf.copy(), boxes.copy()


def host_overlaps(recs, tokens, conf, boxes, eval_type, ignore_dc):
    """Visiting order and overlaps of the host loop: a list of (det index, record or None, overlaps, overlaps_dc)."""
    out = []
    if len(boxes) == 0:
        return out
    for det_idx in np.argsort(-conf):
        rec = Wm.find_rec(recs, tokens[det_idx])
        if rec is None:
            out.append((det_idx, None, None, None))
            continue
        bb = boxes[det_idx].astype(float)
        bbgt, bbgt_dc = rec['boxes'].astype(float), rec['boxes_dc'].astype(float)
        ov_dc = Wm.iou(bbgt_dc, bb, eval_type) if (bbgt_dc.size > 0 and ignore_dc) else None
        ov = Wm.iou(bbgt, bb, eval_type) if bbgt.size > 0 else None
        out.append((det_idx, rec, ov, ov_dc))
    return out


def host_walk(recs, visits, n, ovthresh, ovthresh_dc=0.5):
    """The sequential walk over ``host_overlaps``' visits.  Returns a dict: row_of_det (n,), and per row code, jmax,
    ovmax, ovmax_dc; ``rec['hit']`` is left as the host loop leaves it."""
    for rec in recs:
        rec['hit'][:] = False
    row_of_det = np.full(n, -1, dtype=np.int64)
    code, jm, om, od = [], [], [], []
    for det_idx, rec, ov, ov_dc in visits:
        if rec is None:
            continue
        ovmax, jmax = -np.inf, 0
        ovmax_dc = 0 if ov_dc is None else np.max(ov_dc)
        if ov is not None:
            ovmax, jmax = np.max(ov), int(np.argmax(ov))
        c = NONE
        if ovmax > ovthresh and ovmax_dc < ovthresh_dc:
            if not rec['ignore'][jmax]:
                c = DUP_FP if rec['hit'][jmax] else TP
                rec['hit'][jmax] = True
        elif ov is not None and ovmax_dc < ovthresh_dc:
            c = FP
        row_of_det[det_idx] = len(code)
        code.append(c), jm.append(jmax), om.append(ovmax), od.append(float(ovmax_dc))
    return {'row_of_det': row_of_det, 'code': np.array(code, dtype=np.int64), 'jmax': np.array(jm, dtype=np.int64),
            'ovmax': np.array(om, dtype=np.float64), 'ovmax_dc': np.array(od, dtype=np.float64)}


def threshold_margin(visits, thresholds, ovthresh_dc=0.5):
    """Smallest distance of any host overlap to a matching threshold / of any don't-care overlap to ovthresh_dc."""
    worst = np.inf
    for _, rec, ov, ov_dc in visits:
        if ov is not None:
            for t in thresholds:
                worst = min(worst, np.abs(ov - t).min())
        if ov_dc is not None:
            worst = min(worst, np.abs(ov_dc - ovthresh_dc).min())
    return worst


def write_detfile(path, tokens, conf, boxes):
    """Detections file lines ``idx token score box...`` with values that survive the text round trip (repr)."""
    with open(path, 'w') as fh:
        for i, (t, c, b) in enumerate(zip(tokens, conf, boxes)):
            fh.write("%d %s %r %s\n" % (i, t, float(c), " ".join(repr(float(v)) for v in b)))
