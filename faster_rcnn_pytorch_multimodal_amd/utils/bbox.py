"""Host-side box helpers of the reference's lib/utils/bbox.py that the LiDAR training path needs.

``bbaa_graphics_gems``: axis-aligned BEV rectangle enclosing a yawed 3-D box (Arvo's "Transforming Axis-Aligned
Bounding Boxes", lib/utils/bbox.py:256-293).  It runs on the HOST on the handful of ground-truth boxes of a frame,
exactly where the reference runs it (numpy, inside the data path); the dense 3-D anchor grid gets the same rectangles
from the device (``frcnn_generate_anchors_3d``).
"""
import numpy as np


def bbaa_graphics_gems(bboxes, width=0, height=0, clip=False):
    """(N,>=7) [xc,yc,zc,l,w,h,ry] -> (N,4) [x1,y1,x2,y2].  The rotation matrix keeps the dtype of the boxes, the half
    extents are float64, the per-axis min/max sums are cast to float32 before the centre is added (bbox.py:259-283)."""
    b = np.asarray(bboxes)
    if b.shape[0] == 0:
        return np.zeros((0, 4), dtype=np.float32)
    cos, sin = np.cos(b[:, 6]), np.sin(b[:, 6])
    rot = np.stack((np.stack((cos, sin), 1), np.stack((-sin, cos), 1)), 1)           # (N,2,2) [[c,s],[-s,c]]
    half = np.stack((b[:, 3] / 2.0, b[:, 4] / 2.0), 1).astype(np.float64)
    lo_terms, hi_terms = rot * (-half)[:, None, :], rot * half[:, None, :]
    bmin = np.minimum(lo_terms, hi_terms).sum(2).astype(np.float32) + b[:, 0:2]
    bmax = np.maximum(lo_terms, hi_terms).sum(2).astype(np.float32) + b[:, 0:2]
    out = np.concatenate((bmin[:, 0:1], bmin[:, 1:2], bmax[:, 0:1], bmax[:, 1:2]), 1)
    if clip:                                                                         # _bbox_clip(width-1, height-1)
        out[:, 0::2] = np.clip(out[:, 0::2], 0, width - 1)
        out[:, 1::2] = np.clip(out[:, 1::2], 0, height - 1)
    return out


def bbox_overlaps(boxes, query_boxes):
    """(N,4) x (K,4) device tensors -> (N,K) IoU with the +1 area convention.  lib/utils/bbox.py:5-33."""
    from .. import ops
    return ops.bbox_overlaps(boxes.contiguous(), query_boxes.contiguous())


def bbox_pc_to_voxel_grid(bboxes, bev_extents, info):
    """lib/utils/bbox.py:113-125: metric [xc,yc,zc,l,w,h,ry] rows -> voxel-grid units of the UNSCALED frame, in place."""
    scale = info[6]
    s_info = np.asarray(info[0:6]) * 1 / scale
    kx = (s_info[1] - s_info[0]) / (bev_extents[3] - bev_extents[0])
    ky = (s_info[3] - s_info[2]) / (bev_extents[4] - bev_extents[1])
    bboxes[:, 0] = (bboxes[:, 0] - bev_extents[0]) * kx
    bboxes[:, 1] = (bboxes[:, 1] - bev_extents[1]) * ky
    bboxes[:, 3] = bboxes[:, 3] * kx
    bboxes[:, 4] = bboxes[:, 4] * ky
    return bboxes


def bbox_voxel_grid_to_pc(bboxes, bev_extents, info):
    """lib/utils/bbox.py:140-162, the inverse (host copy of the detections, lib/model/test.py:223-224)."""
    from ..model.test import bbox_voxel_grid_to_pc as impl
    return impl(bboxes, bev_extents, info)


def nms_rotated_host(boxes, scores, thresh, at_equal=True):
    """Rotated BEV NMS on the host in float64: what cfg.TEST.NMS_ROTATED means (not in the reference: the form its authors
    left commented out at lib/utils/filter_predictions.py:56-57), and the rule the device entries frcnn_nms_rotated /
    frcnn_filter_per_class_lidar_rot restate.

    ``boxes`` (N, >=7) [xc,yc,zc,l,w,h,ry], ``scores`` (N,).  The boxes are visited by (score descending, index
    ascending); a box is removed when a KEPT earlier box i has
    ``waymo_eval.iou(bbgt=box_i[None], bb=box_j, 'bev')`` >= ``thresh`` (``at_equal``; the ``>`` of
    ``ops.set_nms_suppress_at_equal(False)`` otherwise) - box j's footprint clipped against box i's; the two argument
    orders differ in the last bits.  ``thresh`` is compared as the float32 the device entries receive, widened to float64.
    A NaN overlap never suppresses.  ``thresh`` <= 0 is refused: disjoint boxes have IoU 0.  Returns the kept indices into
    the input, in visiting order."""
    from ..datasets.waymo_eval import iou
    boxes = np.asarray(boxes, dtype=np.float64)
    scores = np.asarray(scores)
    if boxes.ndim != 2 or boxes.shape[1] < 7 or scores.shape != (boxes.shape[0],):
        raise ValueError("nms_rotated_host: boxes (N, >=7) and scores (N,), got %s and %s" % (boxes.shape, scores.shape))
    t = float(np.float32(thresh))
    if not t > 0.0:
        raise ValueError("nms_rotated_host: thresh %r must be > 0 (disjoint boxes have IoU 0)" % (thresh,))
    order = np.lexsort((np.arange(boxes.shape[0]), -scores))      # score descending, index ascending
    kept = []
    with np.errstate(invalid='ignore', divide='ignore'):
        for j in order:
            if kept:
                ov = iou(boxes[kept][:, :7], boxes[j, :7], 'bev')     # every kept predecessor against box j
                if np.any(ov >= t) if at_equal else np.any(ov > t):
                    continue
            kept.append(int(j))
    return np.asarray(kept, dtype=np.int64)
