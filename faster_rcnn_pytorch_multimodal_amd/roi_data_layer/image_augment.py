"""Image augmentation decisions and their ground-truth side - counterpart of the augmentation block of
``_get_image_blob`` (lib/roi_data_layer/minibatch.py:540-647).

The reference flips the frame with p = 0.5 (:545-556), runs an imgaug pipeline over it and its boxes (:563-600) and then
clips the boxes and flags the ones that left the frame (:614-637).  The split here is the LiDAR one
(``roi_data_layer/lidar_augment.py``): the DECISIONS (a dozen host random numbers) and the gt BOXES (a few rows, float
like the roidb) stay on the host; the PIXELS go through ``ops.image_augment`` (``frcnn_image_augment``, one launch per
stage) with the per-pixel draws coming from the counter-based generator of ``csrc/rng.h`` under ``ImageAugment.seed``, so a
frame is a pure function of its record.

Pinned by the reference's text: the decision tree, the probabilities and the parameter intervals below, the flip's box
formula and the ignore rules.  The pixel operators themselves restate imgaug / cv2 / scikit-image, which are not
available to this project: parity unpinned (``csrc/image_augment.hip`` lists the conventions).

Test time (:648-664, cfg.TEST.AUGMENT_EN): the reference runs ``iaa.imgcorruptlike.Spatter(severity=5)`` over the frame.
Behind cfg.IMAGE.EN_TEST_SPATTER the same split holds: ``draw_test_corruption`` makes the ``Spatter`` record (severity and
the seed of the per-pixel draws) on the host, ``ops.image_spatter`` (``frcnn_image_spatter``, one fused launch) makes the
pixels.  The operator's constants are restated from the published ImageNet-C code: parity unpinned
(``csrc/image_spatter.hip``).
"""
import math
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from ..model.config import cfg
from . import lidar_augment as _shared
from .lidar_augment import set_augmentation_rng  # noqa: F401  (one generator convention for both data layers)

P_FLIP, P_AFFINE, P_DROPOUT = 0.5, 0.3, 0.25                      # :545, :579, :587
MAX_PHOTOMETRIC = 2                                               # SomeOf((0, 2), ...) (:565)
P_FILTER = 0.5                                                    # SomeOf((0, 1), ...) (:566): nothing or one filter
FILTER_KINDS = ('gaussian', 'average', 'median', 'sharpen')       # :567-570
GAUSS_SIGMA_RANGE = (0.5, 2.5)
AVERAGE_K = (1, 2, 3)
MEDIAN_K = (1, 3)                                                 # drawn from {1, 2, 3}; imgaug lowers an even k by one
SHARPEN_ALPHA_RANGE, SHARPEN_LIGHTNESS_RANGE = (0.0, 1.0), (0.75, 1.5)
NOISE_SCALE_RANGE = (0.0, 0.1 * 255)                              # :574
HUE_SAT_RANGE = (-5, 5)                                           # :576, integers, hue and saturation drawn independently
AFFINE_SCALE_RANGE, AFFINE_TRANSLATE_RANGE, AFFINE_SHEAR_RANGE = (0.9, 1.2), (-0.05, 0.05), (-0.05, 0.05)   # :580-584
DROPOUT_P_RANGE, P_DROPOUT_PER_CHANNEL = (0.01, 0.05), 0.5        # :587
# ImageNet-C spatter, mud branch: severity -> (loc, scale, sigma1, thr, sigma2).  PARITY UNPINNED (restated from the
# published code); severities 1-3 are the water branch (Canny edges, distance transform), which is not built
SPATTER_PARAMS = {4: (0.65, 0.3, 1.0, 0.65, 1.5), 5: (0.67, 0.4, 1.0, 0.65, 1.5)}
SPATTER_MUD_COLOUR = (63 / 255.0, 42 / 255.0, 20 / 255.0)         # on memory channels 0, 1, 2 (csrc/image_spatter.hip)
SPATTER_MASK_CUT = 0.8


@dataclass(frozen=True)
class Affine:
    """iaa.Affine's draws (:579-586).  ``translate_*`` are fractions of the width / height, ``shear`` is in DEGREES (what
    imgaug reads the reference's (-0.05, 0.05) as), ``order`` 0 = nearest / 1 = bilinear, ``cval`` the border value."""
    scale_x: float = 1.0
    scale_y: float = 1.0
    translate_x: float = 0.0
    translate_y: float = 0.0
    shear: float = 0.0
    order: int = 1
    cval: int = 0

    def matrix(self, width, height):
        """Forward map (input pixel -> output pixel) as a 3x3 float64 matrix: translate . shear . scale about the centre
        (W/2 - 0.5, H/2 - 0.5), shear in scikit-image's convention [[1, -sin s], [0, cos s]].  The same matrix moves the
        gt corners; its inverse, rounded once to float32, drives the warp."""
        cx, cy = width / 2.0 - 0.5, height / 2.0 - 0.5
        s = math.radians(self.shear)
        to_origin = np.array([[1.0, 0.0, -cx], [0.0, 1.0, -cy], [0.0, 0.0, 1.0]])
        scale = np.array([[self.scale_x, 0.0, 0.0], [0.0, self.scale_y, 0.0], [0.0, 0.0, 1.0]])
        shear = np.array([[1.0, -math.sin(s), 0.0], [0.0, math.cos(s), 0.0], [0.0, 0.0, 1.0]])
        move = np.array([[1.0, 0.0, self.translate_x * width + cx], [0.0, 1.0, self.translate_y * height + cy], [0.0, 0.0, 1.0]])
        return move @ shear @ scale @ to_origin


@dataclass
class ImageAugment:
    """What happens to one frame, in this order: flip, ``stages``, affine, dropout.  ``stages``: the 0-2 members the
    reference's ``SomeOf((0, 2), ..., random_order=True)`` chose, in their drawn order, each a tuple
    ``('none',)`` (the filter group chose nothing), ``('gaussian', sigma)``, ``('average', k)``, ``('median', k)``,
    ``('sharpen', alpha, lightness)``, ``('noise', scale)`` or ``('hue_sat', hue, saturation)``."""
    flip: bool = False
    stages: Tuple[tuple, ...] = ()
    affine: Optional[Affine] = None
    dropout: Optional[Tuple[float, bool]] = None                  # (drop probability, one mask per channel)
    seed: int = 0                                                 # of the per-pixel draws on the device

    @property
    def active_stages(self):
        """The stages that change pixels (a 1x1 average / median and an empty filter group do not)."""
        return tuple(s for s in self.stages if not (s[0] == 'none' or (s[0] in ('average', 'median') and s[1] == 1)))

    @property
    def identity(self):
        return not (self.flip or self.active_stages or self.affine is not None or self.dropout is not None)


@dataclass(frozen=True)
class Spatter:
    """The test-time corruption of one frame (:653): ``severity`` of ``iaa.imgcorruptlike.Spatter`` (4 or 5) and the
    ``seed`` of the per-pixel draws on the device.  A frame is a pure function of (pixels, severity, seed)."""
    severity: int = 5
    seed: int = 0


def spatter_params(severity):
    """``(loc, scale, sigma1, thr, sigma2)`` of a severity.  1-3 are the water branch of the published operator: refused."""
    if severity in (1, 2, 3):
        raise NotImplementedError("Spatter severity %d is the water branch of the published operator (Canny edges, distance "
                                  "transform), which is not built; severities 4 and 5 (mud) are" % severity)
    if severity not in SPATTER_PARAMS:
        raise ValueError("Spatter severity must be 4 or 5 (1-3 are not built), got %r" % (severity,))
    return SPATTER_PARAMS[severity]


def spatter_taps(sigma):
    """Normalised taps of scikit-image / scipy's Gaussian as float32, computed in double: radius int(4 sigma + 0.5)
    (9 taps for sigma 1, 13 for sigma 1.5), exp(-x^2 / 2 sigma^2)."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    taps = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    return (taps / taps.sum()).astype(np.float32)


def draw_test_corruption(rng=None, key=None):
    """The ``Spatter`` record of one test frame: cfg.IMAGE.TEST_SPATTER_SEVERITY and a seed.  ``rng``: a
    ``numpy.random.Generator``; None = the one given to ``set_augmentation_rng``.  Without either, the seed is
    crc32(``key``) continued from cfg.RNG_SEED - ``key`` names the frame (its file) - so a frame's corruption depends on
    the frame and the run's seed alone, not on the order or the rank it is visited in; without a key too, fresh OS entropy
    as everywhere in this module."""
    severity = int(cfg.IMAGE.TEST_SPATTER_SEVERITY)
    spatter_params(severity)
    if rng is None:
        rng = _shared._RNG
    if rng is not None:
        seed = int(rng.integers(0, 1 << 32))
    elif key is not None:
        seed = zlib.crc32(str(key).encode('utf-8'), int(cfg.RNG_SEED) & 0xFFFFFFFF) & 0xFFFFFFFF
    else:
        seed = int(np.random.default_rng().integers(0, 1 << 32))
    return Spatter(severity=severity, seed=seed)


def gaussian_taps(sigma):
    """Normalised taps of the Gaussian blur as float32, computed in double.  Size by imgaug's rule: 3.3 sigma below
    sigma = 3, at least 5, raised to odd (5, 7 or 9 taps over GAUSS_SIGMA_RANGE)."""
    size = max(int(sigma * (3.3 if sigma < 3.0 else 2.9 if sigma < 5.0 else 2.6)), 5)
    size += 1 - size % 2
    x = np.arange(size, dtype=np.float64) - size // 2
    taps = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    return (taps / taps.sum()).astype(np.float32)


def hue_offset(value):
    """imgaug's scaling of a hue value on the [-255, 255] convention to cv2's 0..179 hue circle: int(v / 255 * 90),
    truncated towards zero."""
    return int(float(value) / 255.0 * 90.0)


def _draw_filter(rng):
    if not rng.random() < P_FILTER:
        return ('none',)
    kind = FILTER_KINDS[int(rng.integers(0, len(FILTER_KINDS)))]
    if kind == 'gaussian':
        return (kind, float(rng.uniform(*GAUSS_SIGMA_RANGE)))
    if kind == 'average':
        return (kind, int(AVERAGE_K[int(rng.integers(0, len(AVERAGE_K)))]))
    if kind == 'median':
        k = int(rng.integers(1, 4))
        return (kind, k - 1 if k % 2 == 0 else k)
    return (kind, float(rng.uniform(*SHARPEN_ALPHA_RANGE)), float(rng.uniform(*SHARPEN_LIGHTNESS_RANGE)))


def draw_image_augmentation(width, height, rng=None):
    """The reference's per-frame decisions (:545-597), gated by cfg.IMAGE.EN_AUG_*.  ``rng``: a ``numpy.random.Generator``;
    None = the one given to ``set_augmentation_rng`` or, without one, fresh OS entropy for this frame (:544).  ``width`` and
    ``height`` are part of the signature because the record belongs to one frame size (``Affine.matrix``); no draw
    depends on them."""
    if rng is None:
        rng = _shared._RNG if _shared._RNG is not None else np.random.default_rng()
    aug = ImageAugment()
    if cfg.IMAGE.EN_AUG_FLIP:
        aug.flip = bool(rng.random() < P_FLIP)
    members = [name for name, on in (('filter', cfg.IMAGE.EN_AUG_FILTER), ('noise', cfg.IMAGE.EN_AUG_NOISE),
                                     ('hue_sat', cfg.IMAGE.EN_AUG_HUE_SAT)) if on]
    count = min(int(rng.integers(0, MAX_PHOTOMETRIC + 1)), len(members))
    stages = []
    for j in rng.permutation(len(members))[:count]:
        if members[j] == 'filter':
            stages.append(_draw_filter(rng))
        elif members[j] == 'noise':
            stages.append(('noise', float(rng.uniform(*NOISE_SCALE_RANGE))))
        else:
            stages.append(('hue_sat', int(rng.integers(HUE_SAT_RANGE[0], HUE_SAT_RANGE[1] + 1)),
                           int(rng.integers(HUE_SAT_RANGE[0], HUE_SAT_RANGE[1] + 1))))
    aug.stages = tuple(stages)
    if cfg.IMAGE.EN_AUG_AFFINE and rng.random() < P_AFFINE:
        aug.affine = Affine(scale_x=float(rng.uniform(*AFFINE_SCALE_RANGE)), scale_y=float(rng.uniform(*AFFINE_SCALE_RANGE)),
                            translate_x=float(rng.uniform(*AFFINE_TRANSLATE_RANGE)),
                            translate_y=float(rng.uniform(*AFFINE_TRANSLATE_RANGE)),
                            shear=float(rng.uniform(*AFFINE_SHEAR_RANGE)), order=int(rng.integers(0, 2)),
                            cval=int(rng.integers(0, 256)))
    if cfg.IMAGE.EN_AUG_DROPOUT and rng.random() < P_DROPOUT:
        aug.dropout = (float(rng.uniform(*DROPOUT_P_RANGE)), bool(rng.random() < P_DROPOUT_PER_CHANNEL))
    if not aug.identity:
        aug.seed = int(rng.integers(0, 1 << 32))
    return aug


def augment_image_gt_boxes(entry, aug, width, height):
    """Transform ONE roidb entry in place like the reference transforms ``local_roidb[i]`` and return it: ``boxes`` rows
    [x1, y1, x2, y2] under the flip (:551-554) and the affine map (the four corners moved, their axis-aligned hull taken:
    what imgaug does with bounding boxes), then :614-637 statement by statement - clip to the frame, ``ignore`` set when
    the clipped box is lower or narrower than 2 pixels or keeps less than a tenth of its height, else-if of its width
    (never cleared) - and ``flipped``.  Blur, noise, hue / saturation and dropout do not touch boxes.  The clip and the
    ignore rules run for every record, an identity one included, as in the reference."""
    boxes = entry['boxes']
    entry['flipped'] = bool(aug.flip)                                                # :550,556
    if aug.flip:
        oldx1, oldx2 = boxes[:, 0].copy(), boxes[:, 2].copy()
        boxes[:, 0] = width - oldx2 - 1
        boxes[:, 2] = width - oldx1 - 1
    if aug.affine is not None and len(boxes):
        m = aug.affine.matrix(width, height)
        b = np.asarray(boxes, dtype=np.float64)
        xs = np.stack((b[:, 0], b[:, 2], b[:, 2], b[:, 0]), 1)
        ys = np.stack((b[:, 1], b[:, 1], b[:, 3], b[:, 3]), 1)
        mx = m[0, 0] * xs + m[0, 1] * ys + m[0, 2]
        my = m[1, 0] * xs + m[1, 1] * ys + m[1, 2]
        boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3] = mx.min(1), my.min(1), mx.max(1), my.max(1)
    for j, roi in enumerate(boxes):                                                  # :614-637
        h = roi[3] - roi[1]
        w = roi[2] - roi[0]
        roi[0] = np.minimum(np.maximum(roi[0], 0), width - 1)
        roi[2] = np.minimum(np.maximum(roi[2], 0), width - 1)
        roi[1] = np.minimum(np.maximum(roi[1], 0), height - 1)
        roi[3] = np.minimum(np.maximum(roi[3], 0), height - 1)
        if roi[3] - roi[1] < 2:
            entry['ignore'][j] = True
        if roi[2] - roi[0] < 2:
            entry['ignore'][j] = True
        wc = roi[2] - roi[0]
        hc = roi[3] - roi[1]
        if h != 0 and hc / h < 0.1:
            entry['ignore'][j] = True
        elif w != 0 and wc / w < 0.1:
            entry['ignore'][j] = True
    entry['boxes'] = boxes
    return entry
