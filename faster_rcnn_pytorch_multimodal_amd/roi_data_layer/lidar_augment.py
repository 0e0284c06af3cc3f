"""LiDAR augmentation decisions and their ground-truth side - counterpart of the augmentation block of
``_get_lidar_blob`` (lib/roi_data_layer/minibatch.py:276-425).

The reference decides per frame which transforms run (:284-307), applies them to ~10^5 points and to the few gt boxes
of the roidb entry in numpy.  Here the split is: the DECISIONS (a handful of host random numbers) and the gt BOXES (a few
rows, float64 like the roidb) stay on the host; the POINTS go through ``ops.lidar_augment_points`` (``frcnn_lidar_augment``,
one pass on the device) with the per-point draws coming from the counter-based generator of ``csrc/rng.h`` under
``LidarAugment.seed``, so a frame is a pure function of its record.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from ..model.config import cfg

# probabilities of the reference's np.random.choice draws (:296-307) and the intervals of its parameters (:310-312,322,338)
P_FLIP, P_GAUSS, P_DROPOUT, P_ROTATE, P_SWAP = 0.5, 0.3, 0.3, 0.3, 0.3
SIGMA_XY_MAX, SIGMA_Z_MAX = 0.07, 0.05
P_KEEP_RANGE = (0.8, 1.0)
ROTATION_RANGE = (-np.pi / 2, np.pi / 2)

_RNG = None


def set_augmentation_rng(rng):
    """``numpy.random.Generator`` every later ``draw_lidar_augmentation(rng=None)`` draws from (a repeatable run), or None
    to return to fresh OS entropy per frame (the reference: :284)."""
    global _RNG
    _RNG = rng


@dataclass
class LidarAugment:
    """What happens to one frame.  ``None`` / ``False`` = the step does not run."""
    flip_x: bool = False
    flip_y: bool = False
    gauss: Optional[Tuple[float, float, float]] = None     # (sigma_x, sigma_y, sigma_z) in metres
    p_keep: Optional[float] = None                         # dropout: a point survives with this probability
    rotation: Optional[float] = None                       # radians about z
    swap_xy: bool = False
    rain_rate: Optional[float] = None                      # mm/h (test time)
    rain_max_range: float = 0.0                            # cfg.<DB_NAME>.LIDAR_MAX_RANGE, read with rain_rate
    test_dropout: bool = False                             # test-time dropout, p_keep 0.8
    seed: int = 0                                          # of the per-point draws on the device

    @property
    def identity(self):
        return not (self.flip_x or self.flip_y or self.swap_xy or self.test_dropout or self.gauss is not None
                    or self.p_keep is not None or self.rotation is not None or self.rain_rate is not None)


def _lidar_max_range():
    name = str(cfg.DB_NAME).upper()
    if not name or name not in cfg or 'LIDAR_MAX_RANGE' not in cfg[name]:
        raise ValueError("cfg.TEST.RAIN_SIM_EN needs cfg.DB_NAME ('waymo', 'kitti' or 'cadc') to look up "
                         "cfg.<DB_NAME>.LIDAR_MAX_RANGE; DB_NAME is %r" % cfg.DB_NAME)
    return float(cfg[name].LIDAR_MAX_RANGE)


def draw_lidar_augmentation(rng=None, augment_en=True, mode='train'):
    """The reference's per-frame draws (:284-307 and the parameters at :310-312,322,338), gated by cfg.LIDAR.EN_AUG_*.
    ``augment_en`` switches the training augmentations; ``mode='test'`` adds the rain simulation / test dropout of
    cfg.TEST (:397,422), whatever ``augment_en`` says.  ``rng``: a ``numpy.random.Generator``; None = the one given to
    ``set_augmentation_rng`` or, without one, fresh OS entropy for this frame."""
    if rng is None:
        rng = _RNG if _RNG is not None else np.random.default_rng()
    aug = LidarAugment()
    gauss = dropout = rotate = False
    if augment_en:
        if cfg.LIDAR.EN_AUG_FLIPS:
            aug.flip_y = bool(rng.random() < P_FLIP)
            aug.flip_x = bool(rng.random() < P_FLIP)
        if cfg.LIDAR.EN_AUG_GAUSS_DISTORT:
            gauss = bool(rng.random() < P_GAUSS)
        if cfg.LIDAR.EN_AUG_DROPOUT:
            dropout = bool(rng.random() < P_DROPOUT)
        if cfg.LIDAR.EN_AUG_ROTATE:
            rotate = bool(rng.random() < P_ROTATE)
        if cfg.LIDAR.EN_AUG_SWAP_X_Y:
            aug.swap_xy = bool(rng.random() < P_SWAP)
    if gauss:
        aug.gauss = (float(rng.uniform(0.0, SIGMA_XY_MAX)), float(rng.uniform(0.0, SIGMA_XY_MAX)),
                     float(rng.uniform(0.0, SIGMA_Z_MAX)))
    if dropout:
        aug.p_keep = float(rng.uniform(*P_KEEP_RANGE))
    if rotate:
        aug.rotation = float(rng.uniform(*ROTATION_RANGE))
    if mode == 'test':
        if cfg.TEST.RAIN_SIM_EN:
            aug.rain_rate, aug.rain_max_range = float(cfg.TEST.RAIN_RATE), _lidar_max_range()
        aug.test_dropout = bool(cfg.TEST.DROPOUT_EN)
    if not aug.identity:
        aug.seed = int(rng.integers(0, 1 << 32))
    return aug


def _in_range(box):
    """The reference's per-box range test on the centre (:343-347,364-368)."""
    if (box[0] >= cfg.LIDAR.X_RANGE[0]) & (box[1] >= cfg.LIDAR.Y_RANGE[0]) & (box[2] >= cfg.LIDAR.Z_RANGE[0]):
        if (box[0] < cfg.LIDAR.X_RANGE[1]) & (box[1] < cfg.LIDAR.Y_RANGE[1]) & (box[2] < cfg.LIDAR.Z_RANGE[1]):
            return True
    return False


def augment_gt_boxes(entry, aug):
    """Transform ONE roidb entry in place like the reference transforms ``local_roidb[i]`` and return it: ``boxes`` rows
    [xc, yc, zc, l, w, h, ry] under rotation (:336-348), x/y swap (:352-373) and the flips (:375-395), the ``ignore``
    flags the rotation and the swap recompute from the range test of the moved centre, and ``flipped``.  Restated
    literally (``-(c - mean) + mean``, l / w not exchanged by the swap); Gaussian distortion, dropout and the test-time
    steps do not touch the boxes."""
    boxes = entry['boxes']
    entry['flipped'] = False                                                       # :295
    if aug.rotation is not None:
        cosa, sina = np.cos(np.array([aug.rotation])), np.sin(np.array([aug.rotation]))
        zeros, ones = np.zeros((1,)), np.ones((1,))
        rot = np.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), axis=1).reshape(-1, 3, 3)
        boxes[:, 0:3] = np.matmul(boxes[np.newaxis, :, 0:3], rot)[0]
        boxes[:, 6] += aug.rotation
        for k, box in enumerate(boxes):
            entry['ignore'][k] = not _in_range(box)
    if aug.swap_xy:
        x_range_mean = (cfg.LIDAR.X_RANGE[1] - cfg.LIDAR.X_RANGE[0]) / 2.0
        bx, by = np.copy(boxes[:, 0]), np.copy(boxes[:, 1])
        boxes[:, 0] = by - cfg.LIDAR.Y_RANGE[0]
        boxes[:, 1] = bx - x_range_mean
        boxes[:, 6] = -boxes[:, 6] + np.pi / 2.0
        for k, box in enumerate(boxes):
            entry['ignore'][k] = not _in_range(box)
    if aug.flip_y:
        entry['flipped'] = True
        y_mean = (cfg.LIDAR.Y_RANGE[0] + cfg.LIDAR.Y_RANGE[1]) / 2
        boxes[:, 1] = -(boxes[:, 1].copy() - y_mean) + y_mean
        boxes[:, 6] = -boxes[:, 6].copy()
    if aug.flip_x:
        entry['flipped'] = True
        x_mean = (cfg.LIDAR.X_RANGE[0] + cfg.LIDAR.X_RANGE[1]) / 2
        boxes[:, 0] = -(boxes[:, 0].copy() - x_mean) + x_mean
        boxes[:, 6] = -boxes[:, 6].copy()
    entry['boxes'] = boxes
    return entry
