"""Image augmentation (lib/roi_data_layer/minibatch.py:540-647): the decisions and the gt-box side on the host
(``roi_data_layer/image_augment.py``), the pixels on the device (``frcnn_image_augment``) against a numpy restatement
kept in this file.  imgaug / cv2 / scikit-image are not available, so the pixel operators are PARITY UNPINNED: the
restatement follows the conventions listed in ``csrc/image_augment.hip``.  It is evaluated in float32 with one rounding
per operation where the device result must be bit-equal, and in float64 before rounding where a band is asserted (noise,
hue / saturation); the draws are replayed with the oracle's ``uniform01 / normal01``.

The band ``T_*`` of the float64 comparisons: the largest |device - float64| of the value before rounding measured on
these inputs on an MI355X was 3.73e-5 (noise) and 1.37e-4 (hue / saturation) (profiles/image_augment.md); T = 4 x that,
rounded up.  A pure hue shift (saturation offset 0) is not among the cases: it moves the middle channel by exactly
d / 30, which is a tie (k + 0.5) for every pixel whose max - min is an odd multiple of 15 - a property of the integer
inputs, not of the arithmetic.
"""
import copy
import math

import numpy as np
import pytest
import torch

from faster_rcnn_pytorch_multimodal_amd import _hip, ops
from faster_rcnn_pytorch_multimodal_amd.model import config as C
from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import image_augment as IA
from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.image_augment import (Affine, ImageAugment, augment_image_gt_boxes,
                                                                             draw_image_augmentation, gaussian_taps,
                                                                             hue_offset)
from oracle import frcnn_oracle as O

DEV = "cuda:0"
STREAM = ops.AUG_STREAM
T_NOISE, T_HUE_SAT = 1.5e-4, 5.5e-4
SMALL, FULL = (97, 131), (1280, 1920)
NOISE_CASES = [(3.0, 11), (12.75, 12), (25.5, 13)]                               # (scale, seed)
HUE_SAT_CASES = [(5, -5), (-3, 4), (0, 5), (-4, -2)]                              # (hue, saturation) on imgaug's convention


@pytest.fixture(autouse=True)
def _fresh_cfg():
    C.reset_cfg()
    C.cfg.NET_TYPE = "image"
    IA.set_augmentation_rng(None)
    yield
    IA.set_augmentation_rng(None)
    C.reset_cfg()


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def _frame(shape, seed=0):
    """Noise with constant regions, a one-pixel checkerboard and saturated (0 / 255) patches, some on the border."""
    h, w = shape
    rng = np.random.default_rng(seed)
    im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    im[: h // 4, : w // 3] = (90, 140, 30)
    im[h // 2: h // 2 + h // 5, w // 2:] = 128
    yy, xx = np.mgrid[0: h // 3, 0: w // 4]
    im[h - h // 3:, : w // 4] = (((yy + xx) % 2) * 255).astype(np.uint8)[..., None]
    im[h // 3: h // 3 + 9, w // 3: w // 3 + 11] = 255
    im[: 7, w - 9:] = 0
    im[h - 5:, w - 6:] = 255
    im[h // 4: h // 4 + 6, : 5] = (255, 0, 255)
    return np.ascontiguousarray(im)


def _u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _shifts(img, mode, dt):
    """The nine 3x3 neighbours of every sample, [dy][dx] with offsets -1, 0, 1."""
    h, w = img.shape[:2]
    p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode=mode).astype(dt)
    return [[p[dy:dy + h, dx:dx + w] for dx in range(3)] for dy in range(3)]


def _gauss(img, taps):
    taps = np.asarray(taps, np.float32)
    r, (h, w) = len(taps) // 2, img.shape[:2]
    p = np.pad(img, ((r, r), (r, r), (0, 0)), mode='reflect').astype(np.float32)
    acc = taps[0] * p[:, 0:w]
    for k in range(1, len(taps)):
        acc = acc + taps[k] * p[:, k:k + w]
    out = taps[0] * acc[0:h]
    for k in range(1, len(taps)):
        out = out + taps[k] * acc[k:k + h]
    assert out.dtype == np.float32
    return _u8(out)


def _average(img, k):
    s = _shifts(img, 'reflect', np.int64)
    window = [s[dy][dx] for dy in range(3) for dx in range(3)] if k == 3 else [s[0][0], s[0][1], s[1][0], s[1][1]]
    return _u8(sum(window) / float(k * k))


def _median(img):
    s = _shifts(img, 'edge', np.int64)
    return np.sort(np.stack([s[dy][dx] for dy in range(3) for dx in range(3)], 0), 0)[4].astype(np.uint8)


def _sharpen(img, alpha, lightness):
    wc, wn = np.float32((1.0 - alpha) + alpha * (8.0 + lightness)), np.float32(-alpha)
    s = _shifts(img, 'reflect', np.int64)
    neigh = sum(s[dy][dx] for dy in range(3) for dx in range(3) if (dy, dx) != (1, 1))
    return _u8(wc * s[1][1].astype(np.float32) + wn * neigh.astype(np.float32))


def _noise_pre(img, scale, seed):
    """float64 value before rounding: px + s * normal01, the device's Box-Muller expression in double."""
    h, w = img.shape[:2]
    idx = np.arange(h * w)
    out = np.empty((h * w, 3), np.float64)
    two_pi = np.float64(np.float32(6.2831853071795864))
    for c in range(3):
        k = STREAM['image_noise_%d' % c]
        u1 = O.uniform01(seed, 2 * k, idx).astype(np.float64)
        u2 = O.uniform01(seed, 2 * k + 1, idx).astype(np.float64)
        out[:, c] = img.reshape(-1, 3)[:, c] + np.float64(np.float32(scale)) * (np.sqrt(-2.0 * np.log(u1)) * np.cos(two_pi * u2))
    return out.reshape(h, w, 3)


def _hue_sat_pre(img, hue, sat):
    """float64 value before rounding; memory channel 0 plays R (the reference hands a BGR frame to an RGB augmenter)."""
    r, g, b = (img[..., c].astype(np.float64) for c in range(3))
    v, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    d = v - mn
    safe_d, safe_v = np.where(d > 0, d, 1.0), np.where(v > 0, v, 1.0)
    s = np.where(v > 0, 255.0 * d / safe_v, 0.0)
    hh = np.where(v == r, 60.0 * (g - b) / safe_d, np.where(v == g, 120.0 + 60.0 * (b - r) / safe_d, 240.0 + 60.0 * (r - g) / safe_d))
    hh = np.where(hh < 0, hh + 360.0, hh) * 0.5
    hh = np.where(d > 0, hh, 0.0) + float(hue_offset(hue))
    hh = np.where(hh < 0, hh + 180.0, hh)
    hh = np.where(hh >= 180.0, hh - 180.0, hh)
    s = np.clip(s + float(sat), 0.0, 255.0) / 255.0
    h6 = hh / 30.0
    sector = np.floor(h6)
    f = h6 - sector
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    table = {0: (v, t, p), 1: (q, v, p), 2: (p, v, t), 3: (p, q, v), 4: (t, p, v), 5: (v, p, q)}
    out = np.empty(img.shape, np.float64)
    for c in range(3):
        out[..., c] = np.select([sector == k for k in range(6)], [table[k][c] for k in range(6)], default=table[5][c])
    return out


def _affine(img, affine):
    h, w = img.shape[:2]
    m = np.linalg.inv(affine.matrix(w, h)).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    xs, ys = (m[0, 0] * x + m[0, 1] * y) + m[0, 2], (m[1, 0] * x + m[1, 1] * y) + m[1, 2]
    assert xs.dtype == np.float32
    cval = np.float32(affine.cval)

    def tap(yi, xi):
        inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        got = img[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)].astype(np.float32)
        return np.where(inside[..., None], got, cval)

    if affine.order == 0:
        return tap(np.rint(ys).astype(np.int64), np.rint(xs).astype(np.int64)).astype(np.uint8)
    xf, yf = np.floor(xs), np.floor(ys)
    fx, fy = (xs - xf)[..., None], (ys - yf)[..., None]
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    one = np.float32(1.0)
    top = tap(yi, xi) * (one - fx) + tap(yi, xi + 1) * fx
    bot = tap(yi + 1, xi) * (one - fx) + tap(yi + 1, xi + 1) * fx
    out = top * (one - fy) + bot * fy
    assert out.dtype == np.float32
    return _u8(out)


def _dropout(img, p, per_channel, seed):
    h, w = img.shape[:2]
    if per_channel:
        drop = (O.uniform01(seed, STREAM['image_dropout'], np.arange(h * w * 3)) < np.float32(p)).reshape(h, w, 3)
    else:
        drop = (O.uniform01(seed, STREAM['image_dropout'], np.arange(h * w)) < np.float32(p)).reshape(h, w, 1)
    return np.where(drop, 0, img).astype(np.uint8)


def _restate(img, aug):
    """The whole record, every stage uint8 -> uint8.  Noise and hue / saturation are rounded from the float64 value, so a
    record that holds them is equal to the device only outside the band."""
    im = img[:, ::-1].copy() if aug.flip else img.copy()
    for st in aug.active_stages:
        if st[0] == 'gaussian':
            im = _gauss(im, gaussian_taps(st[1]))
        elif st[0] == 'average':
            im = _average(im, st[1])
        elif st[0] == 'median':
            im = _median(im)
        elif st[0] == 'sharpen':
            im = _sharpen(im, st[1], st[2])
        elif st[0] == 'noise':
            im = _u8(_noise_pre(im, st[1], aug.seed))
        else:
            im = _u8(_hue_sat_pre(im, st[1], st[2]))
    if aug.affine is not None:
        im = _affine(im, aug.affine)
    if aug.dropout is not None:
        im = _dropout(im, aug.dropout[0], aug.dropout[1], aug.seed)
    return im


def _band_share(v, t):
    """Share of samples whose float64 value lies within t of a rounding boundary (k + 0.5) after the clip."""
    c = np.clip(v, 0.0, 255.0)
    return float((np.abs(c - np.floor(c) - 0.5) <= t).mean())


def _entry(filename="frame.npy", boxes=None):
    boxes = np.array([[10.0, 12.0, 60.0, 70.0], [40.0, 30.0, 125.0, 90.0], [2.0, 3.0, 30.0, 20.0], [70.0, 50.0, 100.0, 80.0]],
                     np.float32) if boxes is None else np.asarray(boxes, np.float32)
    n = len(boxes)
    return {"filename": filename, "boxes": boxes, "gt_classes": np.ones(n, np.int64), "ignore": np.zeros(n, np.int64),
            "boxes_dc": np.zeros((0, 4), np.float32), "flipped": False}


# ---------------------------------------------------------------------------------------------------------------
# CPU: decisions
# ---------------------------------------------------------------------------------------------------------------
def _within(freq, p, n, what):
    assert abs(freq - p) <= 4 * math.sqrt(p * (1 - p) / n), (what, freq, p)


def _both_halves(values, lo, hi, what):
    values = np.asarray(values, np.float64)
    assert len(values) and values.min() >= lo and values.max() <= hi, (what, values.min(), values.max())
    mid = (lo + hi) / 2
    assert (values < mid).any() and (values > mid).any(), what


def test_draws_follow_the_reference_decision_tree():
    n = 20000
    rng = np.random.default_rng(2025)
    draws = [draw_image_augmentation(1920, 1280, rng) for _ in range(n)]
    _within(np.mean([d.flip for d in draws]), 0.5, n, "flip")
    _within(np.mean([d.affine is not None for d in draws]), 0.3, n, "affine")
    _within(np.mean([d.dropout is not None for d in draws]), 0.25, n, "dropout")
    for count in (0, 1, 2):
        _within(np.mean([len(d.stages) == count for d in draws]), 1 / 3, n, "stage count %d" % count)
    member = lambda st: 'filter' if st[0] in ('none',) + IA.FILTER_KINDS else st[0]
    pairs = set()
    for d in draws:
        names = [member(st) for st in d.stages]
        assert len(names) <= 2 and len(set(names)) == len(names), d.stages          # no member twice in a frame
        if len(names) == 2:
            pairs.add(tuple(names))
    assert pairs == {(a, b) for a in ('filter', 'noise', 'hue_sat') for b in ('filter', 'noise', 'hue_sat') if a != b}
    # every member equally likely: P(member in frame) = (0 + 1/3 + 2/3) / 3 = 1/3
    for name in ('filter', 'noise', 'hue_sat'):
        _within(np.mean([name in [member(st) for st in d.stages] for d in draws]), 1 / 3, n, name)
    filters = [st for d in draws for st in d.stages if member(st) == 'filter']
    nf = len(filters)
    _within(np.mean([st[0] == 'none' for st in filters]), 0.5, nf, "filter group empty")
    for kind in IA.FILTER_KINDS:
        _within(np.mean([st[0] == kind for st in filters]), 0.125, nf, kind)
    med = [st[1] for st in filters if st[0] == 'median']
    assert set(med) == {1, 3}
    _within(np.mean([k == 3 for k in med]), 1 / 3, len(med), "median k = 3")
    avg = [st[1] for st in filters if st[0] == 'average']
    assert set(avg) == {1, 2, 3}
    for k in (1, 2, 3):
        _within(np.mean([v == k for v in avg]), 1 / 3, len(avg), "average k")
    _both_halves([st[1] for st in filters if st[0] == 'gaussian'], 0.5, 2.5, "sigma")
    assert {len(gaussian_taps(st[1])) for st in filters if st[0] == 'gaussian'} == {5, 7, 9}
    _both_halves([st[1] for st in filters if st[0] == 'sharpen'], 0.0, 1.0, "alpha")
    _both_halves([st[2] for st in filters if st[0] == 'sharpen'], 0.75, 1.5, "lightness")
    noise = [st[1] for d in draws for st in d.stages if st[0] == 'noise']
    _both_halves(noise, 0.0, 0.1 * 255, "noise scale")
    hs = np.array([st[1:] for d in draws for st in d.stages if st[0] == 'hue_sat'])
    assert set(hs[:, 0]) == set(range(-5, 6)) and set(hs[:, 1]) == set(range(-5, 6))
    assert abs(np.corrcoef(hs[:, 0], hs[:, 1])[0, 1]) < 4 / math.sqrt(len(hs))      # two independent draws
    aff = [d.affine for d in draws if d.affine is not None]
    _both_halves([a.scale_x for a in aff], 0.9, 1.2, "scale x")
    _both_halves([a.scale_y for a in aff], 0.9, 1.2, "scale y")
    assert abs(np.corrcoef([a.scale_x for a in aff], [a.scale_y for a in aff])[0, 1]) < 4 / math.sqrt(len(aff))
    _both_halves([a.translate_x for a in aff], -0.05, 0.05, "translate x")
    _both_halves([a.translate_y for a in aff], -0.05, 0.05, "translate y")
    _both_halves([a.shear for a in aff], -0.05, 0.05, "shear (degrees)")
    _within(np.mean([a.order == 1 for a in aff]), 0.5, len(aff), "order")
    assert {a.order for a in aff} == {0, 1}
    cvals = [a.cval for a in aff]
    assert all(isinstance(c, int) for c in cvals)
    _both_halves(cvals, 0, 255, "cval")
    drop = [d.dropout for d in draws if d.dropout is not None]
    _both_halves([p for p, _ in drop], 0.01, 0.05, "dropout p")
    _within(np.mean([pc for _, pc in drop]), 0.5, len(drop), "dropout per channel")
    for d in draws:
        assert 0 <= d.seed < 2 ** 32
        if d.identity:
            assert d.seed == 0 and not d.flip and d.affine is None and d.dropout is None and not d.active_stages
    assert any(d.identity for d in draws) and any(d.identity and d.stages for d in draws)
    # repeatable with a generator; rng=None reads the generator installed for the run (shared with the LiDAR module)
    a = [draw_image_augmentation(100, 80, np.random.default_rng(4)) for _ in range(2)]
    assert a[0] == a[1]
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_augment
    assert IA.set_augmentation_rng is lidar_augment.set_augmentation_rng
    IA.set_augmentation_rng(np.random.default_rng(4))
    assert draw_image_augmentation(100, 80) == a[0]
    IA.set_augmentation_rng(None)
    assert len({draw_image_augmentation(100, 80).seed for _ in range(12)}) > 1


def test_per_step_switches():
    cfg = C.cfg.IMAGE
    assert cfg.EN_AUG is False
    assert all(cfg[k] is True for k in ("EN_AUG_FLIP", "EN_AUG_FILTER", "EN_AUG_NOISE", "EN_AUG_HUE_SAT", "EN_AUG_AFFINE",
                                        "EN_AUG_DROPOUT"))
    rng = np.random.default_rng(1)
    member_of = {"EN_AUG_FILTER": ('none',) + IA.FILTER_KINDS, "EN_AUG_NOISE": ('noise',), "EN_AUG_HUE_SAT": ('hue_sat',)}
    for key in ("EN_AUG_FLIP", "EN_AUG_FILTER", "EN_AUG_NOISE", "EN_AUG_HUE_SAT", "EN_AUG_AFFINE", "EN_AUG_DROPOUT"):
        C.reset_cfg()
        C.cfg.IMAGE[key] = False
        draws = [draw_image_augmentation(64, 48, rng) for _ in range(600)]
        if key == "EN_AUG_FLIP":
            assert not any(d.flip for d in draws) and any(d.affine for d in draws)
        elif key == "EN_AUG_AFFINE":
            assert all(d.affine is None for d in draws) and any(d.flip for d in draws)
        elif key == "EN_AUG_DROPOUT":
            assert all(d.dropout is None for d in draws) and any(d.flip for d in draws)
        else:
            kinds = {st[0] for d in draws for st in d.stages}
            assert not kinds & set(member_of[key]) and kinds
    C.reset_cfg()
    for key in ("EN_AUG_FLIP", "EN_AUG_FILTER", "EN_AUG_NOISE", "EN_AUG_HUE_SAT", "EN_AUG_AFFINE", "EN_AUG_DROPOUT"):
        C.cfg.IMAGE[key] = False
    for _ in range(50):
        d = draw_image_augmentation(64, 48, rng)
        assert d == ImageAugment() and d.identity and d.seed == 0
    C.cfg_from_list(["IMAGE.EN_AUG", "True", "IMAGE.EN_AUG_NOISE", "True"])
    assert C.cfg.IMAGE.EN_AUG is True and C.cfg.IMAGE.EN_AUG_NOISE is True


def test_gaussian_taps_and_hue_offset():
    for sigma, size in ((0.5, 5), (1.0, 5), (1.6, 5), (1.9, 7), (2.2, 7), (2.45, 9), (2.5, 9)):
        taps = gaussian_taps(sigma)
        assert taps.dtype == np.float32 and len(taps) == size and abs(float(taps.astype(np.float64).sum()) - 1) < 1e-6
        np.testing.assert_array_equal(taps, taps[::-1])
        x = np.arange(size) - size // 2
        np.testing.assert_allclose(taps[1:] / taps[:-1], np.exp(-(x[1:] ** 2 - x[:-1] ** 2) / (2 * sigma ** 2)), rtol=1e-5)
    assert [hue_offset(v) for v in range(-5, 6)] == [-1, -1, -1, 0, 0, 0, 0, 0, 1, 1, 1]
    assert hue_offset(255) == 90 and hue_offset(-255) == -90


# ---------------------------------------------------------------------------------------------------------------
# CPU: boxes
# ---------------------------------------------------------------------------------------------------------------
def test_flip_moves_boxes_by_the_reference_formula():
    w, h = 200, 100
    rows = [[10.0, 5.0, 60.0, 40.0], [0.0, 0.0, 199.0, 99.0], [150.5, 20.0, 180.25, 90.0]]
    e = augment_image_gt_boxes(_entry(boxes=rows), ImageAugment(flip=True), w, h)
    np.testing.assert_array_equal(e['boxes'], np.array([[139.0, 5.0, 189.0, 40.0], [0.0, 0.0, 199.0, 99.0],
                                                        [18.75, 20.0, 48.5, 90.0]], np.float32))
    assert e['flipped'] is True and not e['ignore'].any()
    augment_image_gt_boxes(e, ImageAugment(flip=True), w, h)                        # twice = identity
    np.testing.assert_array_equal(e['boxes'], np.asarray(rows, np.float32))
    e64 = _entry(boxes=rows)
    e64['boxes'] = e64['boxes'].astype(np.float64)
    assert augment_image_gt_boxes(e64, ImageAugment(flip=True), w, h)['boxes'].dtype == np.float64
    plain = augment_image_gt_boxes(_entry(boxes=rows), ImageAugment(stages=(('noise', 3.0),), dropout=(0.02, True)), w, h)
    np.testing.assert_array_equal(plain['boxes'], np.asarray(rows, np.float32))     # photometric steps leave boxes alone
    assert plain['flipped'] is False


def test_affine_moves_the_corners_and_takes_their_hull():
    w, h = 320, 240
    aff = Affine(scale_x=1.15, scale_y=0.93, translate_x=0.04, translate_y=-0.03, shear=0.05, order=1, cval=7)
    m = aff.matrix(w, h)
    centre = np.array([w / 2 - 0.5, h / 2 - 0.5, 1.0])
    np.testing.assert_allclose(m @ centre, centre + [0.04 * w, -0.03 * h, 0.0], atol=1e-9)      # the centre only translates
    s = math.radians(0.05)
    np.testing.assert_allclose(m[:2, :2], [[1.15, -0.93 * math.sin(s)], [0.0, 0.93 * math.cos(s)]], atol=1e-12)
    e0 = _entry(boxes=[[50.0, 60.0, 150.0, 140.0], [100.0, 30.0, 260.0, 200.0]])
    e = augment_image_gt_boxes(copy.deepcopy(e0), ImageAugment(affine=aff), w, h)
    for k, (x1, y1, x2, y2) in enumerate(e0['boxes'].astype(np.float64)):
        corners = np.array([[x1, y1, 1], [x2, y1, 1], [x2, y2, 1], [x1, y2, 1]], np.float64) @ m.T
        want = [corners[:, 0].min(), corners[:, 1].min(), corners[:, 0].max(), corners[:, 1].max()]
        np.testing.assert_allclose(e['boxes'][k], np.asarray(want, np.float32), rtol=0, atol=1e-4)
    assert not e['ignore'].any() and e['flipped'] is False
    # flip first, then the map (the order of the reference)
    both = augment_image_gt_boxes(copy.deepcopy(e0), ImageAugment(flip=True, affine=aff), w, h)
    flipped = augment_image_gt_boxes(copy.deepcopy(e0), ImageAugment(flip=True), w, h)
    np.testing.assert_array_equal(both['boxes'], augment_image_gt_boxes(flipped, ImageAugment(affine=aff), w, h)['boxes'])


def test_ignore_rules():
    w, h = 200, 100
    # translate by +90 % of the width is outside the reference's range, but makes every rule reachable with round numbers
    right = Affine(translate_x=0.45)                                                 # +90 px
    down = Affine(translate_y=0.45)                                                  # +45 px
    rows = [[20.0, 10.0, 60.0, 40.0]]
    ok = augment_image_gt_boxes(_entry(boxes=rows), ImageAugment(affine=Affine(translate_x=0.05)), w, h)
    np.testing.assert_allclose(ok['boxes'], [[30.0, 10.0, 70.0, 40.0]], atol=1e-4)
    assert not ok['ignore'].any()                                                    # a box that triggers none
    # clipped width < 2: x in [108.5, 110] -> [198.5, 199]
    e = augment_image_gt_boxes(_entry(boxes=[[108.5, 10.0, 110.0, 40.0]]), ImageAugment(affine=right), w, h)
    np.testing.assert_allclose(e['boxes'], [[198.5, 10.0, 199.0, 40.0]], atol=1e-4)
    assert e['ignore'][0]
    # clipped height < 2
    e = augment_image_gt_boxes(_entry(boxes=[[20.0, 53.0, 60.0, 54.5]]), ImageAugment(affine=down), w, h)
    np.testing.assert_allclose(e['boxes'], [[20.0, 98.0, 60.0, 99.0]], atol=1e-4)
    assert e['ignore'][0]
    # hc / h < 0.1 with the clipped height still >= 2: h = 40, clipped to 3
    e = augment_image_gt_boxes(_entry(boxes=[[20.0, 51.0, 60.0, 91.0]]), ImageAugment(affine=down), w, h)
    np.testing.assert_allclose(e['boxes'], [[20.0, 96.0, 60.0, 99.0]], atol=1e-4)
    assert e['ignore'][0]
    # the else-if on wc / w: w = 60, clipped to 4, height untouched
    e = augment_image_gt_boxes(_entry(boxes=[[105.0, 10.0, 165.0, 40.0]]), ImageAugment(affine=right), w, h)
    np.testing.assert_allclose(e['boxes'], [[195.0, 10.0, 199.0, 40.0]], atol=1e-4)
    assert e['ignore'][0]
    # just above the tenth: w = 30 clipped to 4 (ratio 0.133): kept
    e = augment_image_gt_boxes(_entry(boxes=[[105.0, 10.0, 135.0, 40.0]]), ImageAugment(affine=right), w, h)
    assert not e['ignore'][0]
    # a box entirely outside collapses onto the border: ignored
    e = augment_image_gt_boxes(_entry(boxes=[[150.0, 10.0, 190.0, 40.0]]), ImageAugment(affine=right), w, h)
    np.testing.assert_allclose(e['boxes'], [[199.0, 10.0, 199.0, 40.0]], atol=1e-4)
    assert e['ignore'][0]
    # ignore is only ever set
    e = _entry(boxes=rows)
    e['ignore'][0] = 1
    assert augment_image_gt_boxes(e, ImageAugment(flip=True), w, h)['ignore'][0] == 1
    assert augment_image_gt_boxes(e, ImageAugment(), w, h)['ignore'][0] == 1
    # the roidb entry handed in is the one modified and returned
    e = _entry(boxes=rows)
    assert augment_image_gt_boxes(e, ImageAugment(flip=True), w, h) is e


# ---------------------------------------------------------------------------------------------------------------
# CPU: ABI, gate, the band
# ---------------------------------------------------------------------------------------------------------------
def test_image_augment_argument_errors_are_reported_without_a_gpu():
    import ctypes
    lib = _hip.load()
    assert lib.frcnn_version() >= 111
    h, w = 48, 64
    need = lib.frcnn_image_augment_ws_bytes(h, w)
    assert need >= h * w * 3 and lib.frcnn_image_augment_ws_bytes(0, 5) == 0
    img, out, scr = 1 << 20, 2 << 20, 3 << 20                    # non-null device addresses: never dereferenced on the host

    def call(img=img, h=h, w=w, flip=0, stages=((ops.IMG_MEDIAN, []),), scratch=scr, scratch_bytes=need, out=out, n=None,
             codes="auto", params="auto", pre=None):
        flat = []
        for _, vals in stages:
            flat += list(vals) + [0.0] * (ops.IMG_NUM_PARAMS - len(vals))
        c = (ctypes.c_int * max(len(stages), 1))(*[s[0] for s in stages]) if codes == "auto" else codes
        p = _hip.float_array(flat or [0.0]) if params == "auto" else params
        return lib.frcnn_image_augment(img, h, w, flip, len(stages) if n is None else n, c, p, 1, None, scratch, scratch_bytes,
                                       out, pre, None)

    two = ((ops.IMG_MEDIAN, []), (ops.IMG_NOISE, [3.0]))
    for kw in (dict(img=None), dict(out=None), dict(codes=None), dict(params=None), dict(stages=two, scratch=None)):
        assert call(**kw) == -1 and b"null" in lib.frcnn_last_error(), kw
    for kw in (dict(h=0), dict(w=0), dict(h=-3), dict(w=-1)):
        assert call(**kw) == -1 and b"frame size" in lib.frcnn_last_error(), kw
    assert call(stages=((9, []),)) == -1 and b"unknown stage code 9" in lib.frcnn_last_error()
    assert call(stages=((ops.IMG_MEDIAN, []), (-1, []))) == -1 and b"unknown stage code" in lib.frcnn_last_error()
    assert call(stages=two, scratch_bytes=need - 1) == -1 and b"scratch too small" in lib.frcnn_last_error()
    assert call(stages=two, scratch_bytes=0) == -1
    assert call(n=ops.IMG_MAX_STAGES + 1) == -1 and b"num_stages" in lib.frcnn_last_error()
    assert call(flip=2) == -1
    # aliasing: the three buffers must be distinct
    assert call(out=img) == -1 and b"overlap" in lib.frcnn_last_error()
    assert call(out=img + 100) == -1
    assert call(stages=two, scratch=out) == -1 and b"scratch must not overlap" in lib.frcnn_last_error()
    assert call(stages=two, scratch=img + 64) == -1
    # stage parameters
    assert call(stages=((ops.IMG_GAUSS, [4.0] + [0.25] * 4),)) == -1 and b"taps" in lib.frcnn_last_error()
    assert call(stages=((ops.IMG_AVERAGE, [1.0]),)) == -1 and b"average" in lib.frcnn_last_error()
    assert call(stages=((ops.IMG_NOISE, [-1.0]),)) == -1
    assert call(stages=((ops.IMG_NOISE, [float("nan")]),)) == -1 and b"non-finite" in lib.frcnn_last_error()
    assert call(stages=((ops.IMG_AFFINE, [1, 0, 0, 0, 1, 0, 2, 0]),)) == -1 and b"affine" in lib.frcnn_last_error()
    assert call(stages=((ops.IMG_AFFINE, [1, 0, 0, 0, 1, 0, 1, 256]),)) == -1
    assert call(stages=((ops.IMG_DROPOUT, [1.5, 0]),)) == -1 and b"dropout" in lib.frcnn_last_error()
    assert call(pre=4 << 20) == -1 and b"debug_pre" in lib.frcnn_last_error()
    with pytest.raises(_hip.HipError, match="no CPU path"):
        ops.image_augment(torch.zeros(8, 8, 3, dtype=torch.uint8), ImageAugment(flip=True))


def test_stage_lists_of_a_record():
    aug = ImageAugment(flip=True, stages=(('none',), ('average', 1)), seed=3)
    assert aug.identity is False and aug.active_stages == ()
    assert ops.image_augment_stages(aug, 48, 64) == (True, [])
    aug = ImageAugment(stages=(('hue_sat', 5, -4), ('gaussian', 2.5)), affine=Affine(order=0, cval=9), dropout=(0.03, True))
    flip, stages = ops.image_augment_stages(aug, 48, 64)
    assert flip is False and [c for c, _ in stages] == [ops.IMG_HUE_SAT, ops.IMG_GAUSS, ops.IMG_AFFINE, ops.IMG_DROPOUT]
    assert stages[0][1] == [1.0, -4.0] and stages[1][1][0] == 9 and len(stages[1][1]) == 10
    np.testing.assert_allclose(stages[2][1], [1, 0, 0, 0, 1, 0, 0, 9], atol=1e-12)
    assert stages[3][1] == [0.03, 1.0]
    assert ImageAugment(stages=(('median', 1),)).identity and not ImageAugment(stages=(('median', 3),)).identity
    assert max(len(v) for _, v in stages) <= ops.IMG_NUM_PARAMS


def test_gate(tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import minibatch
    path = str(tmp_path / "frame.npy")
    np.save(path, _frame((32, 48)))
    with pytest.raises(NotImplementedError, match=r"cfg\.IMAGE\.EN_AUG"):
        minibatch._get_image_blob([_entry(path)], 1.0, augment_en=True, device='cpu')
    for on in (False, True):
        C.cfg.IMAGE.EN_AUG = on
        with pytest.raises(NotImplementedError, match="Spatter"):
            minibatch._get_image_blob([path], 1.0, augment_en=True, mode='test', device='cpu')


def test_restatement_is_self_consistent():
    """What the GPU tests compare against, checked on the CPU: stages that must not change a frame do not, the median
    network's definition, and the share of samples the float64 comparisons leave unpinned (< 1 % on every case)."""
    im = _frame(SMALL, 1)
    flat = np.full((20, 30, 3), 77, np.uint8)
    for got in (_gauss(flat, gaussian_taps(2.5)), _average(flat, 2), _average(flat, 3), _median(flat), _sharpen(flat, 0.7, 1.0),
                _affine(flat, Affine(order=1, cval=77, scale_x=1.1, translate_y=0.04))):
        np.testing.assert_array_equal(got, flat)
    np.testing.assert_array_equal(_affine(im, Affine(order=0)), im)
    np.testing.assert_array_equal(_affine(im, Affine(order=1)), im)
    np.testing.assert_array_equal(_u8(_hue_sat_pre(im, 0, 0)), im)                  # RGB -> HSV -> RGB
    np.testing.assert_array_equal(_sharpen(im, 0.0, 1.2), im)
    np.testing.assert_array_equal(_u8(_noise_pre(im, 0.0, 5)), im)
    assert np.array_equal(_u8(np.array([0.5, 1.5, 2.5, -3.0, 300.0])), [0, 2, 2, 0, 255])   # half to even, clip
    assert np.array_equal(_average(np.array([[[1], [2]], [[3], [4]]], np.uint8), 2)[..., 0], [[2, 2], [2, 2]])   # 10 / 4 = 2.5 -> 2
    for shape in (SMALL, FULL):
        frame = _frame(shape, 1)
        for scale, seed in (NOISE_CASES if shape == SMALL else NOISE_CASES[-1:]):
            v = _noise_pre(frame, scale, seed)
            assert _band_share(v, T_NOISE) < 0.01, (shape, scale)
            assert abs(float((v - frame).std()) - scale) < 0.05 * scale
        for hue, sat in (HUE_SAT_CASES if shape == SMALL else HUE_SAT_CASES[:1]):
            assert _band_share(_hue_sat_pre(frame, hue, sat), T_HUE_SAT) < 0.01, (shape, hue, sat)


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def _run(img, aug, **kw):
    dev = torch.from_numpy(img).to(DEV)
    out = ops.image_augment(dev, aug, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), torch.from_numpy(img))                            # the input is not touched
    return out.cpu().numpy()


def _assert_same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d samples differ, first at %s: got %d want %d" % (
        what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


EXACT = {
    "flip": ImageAugment(flip=True),
    "average2": ImageAugment(stages=(('average', 2),)),
    "average3": ImageAugment(stages=(('average', 3),)),
    "median": ImageAugment(stages=(('median', 3),)),
    "dropout_shared": ImageAugment(dropout=(0.05, False), seed=21),
    "dropout_per_channel": ImageAugment(dropout=(0.03, True), seed=22),
    "affine_nearest": ImageAugment(affine=Affine(1.17, 0.92, 0.04, -0.05, 0.05, 0, 200)),
    "affine_nearest_shrink": ImageAugment(affine=Affine(0.9, 0.9, -0.05, 0.05, -0.05, 0, 0)),
    "gauss5": ImageAugment(stages=(('gaussian', 1.0),)),
    "gauss7": ImageAugment(stages=(('gaussian', 2.0),)),
    "gauss9": ImageAugment(stages=(('gaussian', 2.5),)),
    "sharpen": ImageAugment(stages=(('sharpen', 0.8, 1.3),)),
    "sharpen_dark": ImageAugment(stages=(('sharpen', 0.35, 0.75),)),
    "affine_bilinear": ImageAugment(affine=Affine(1.2, 0.95, -0.03, 0.05, -0.05, 1, 90)),
    "affine_bilinear_shrink": ImageAugment(affine=Affine(0.9, 0.9, 0.05, -0.05, 0.05, 1, 255)),
    "flip_median": ImageAugment(flip=True, stages=(('median', 3),)),
    "flip_gauss9": ImageAugment(flip=True, stages=(('gaussian', 2.5),)),
    "flip_affine_bilinear": ImageAugment(flip=True, affine=Affine(1.1, 1.1, 0.02, 0.02, 0.05, 1, 3)),
}
FULL_EXACT = ("median", "gauss9", "affine_bilinear", "dropout_per_channel", "flip")     # one per stage family


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(EXACT))
def test_exact_stages_are_bit_equal_to_the_restatement(hip, case):
    aug = EXACT[case]
    assert len(ops.image_augment_stages(aug, *SMALL)[1]) <= 1
    for shape in (SMALL, (16, 64), (17, 65), (5, 7)) + ((FULL,) if case in FULL_EXACT else ()):
        im = _frame(shape, 2) if min(shape) > 8 else np.random.default_rng(0).integers(0, 256, shape + (3,), dtype=np.uint8)
        want = _restate(im, aug)
        got = _run(im, aug)
        _assert_same(got, want, "%s %s" % (case, shape))
        if shape == SMALL and case != "affine_nearest_shrink":
            assert (got != im).mean() > (0.01 if "dropout" in case else 0.2)        # the stage did something


def _check_band(got, v, t, what):
    c = np.clip(v, 0.0, 255.0)
    pinned = np.abs(c - np.floor(c) - 0.5) > t
    want = _u8(v)
    assert (1.0 - pinned.mean()) < 0.01, what
    _assert_same(np.where(pinned, got, 0), np.where(pinned, want, 0), what)
    lo, hi = np.floor(c), np.ceil(c)
    assert (((got == lo) | (got == hi)) | pinned).all(), what


def _pre_and_bytes(im, aug):
    dev = torch.from_numpy(im).to(DEV)
    pre = torch.full(im.shape, float("nan"), dtype=torch.float32, device=DEV)
    got = ops.image_augment(dev, aug, debug_pre=pre).cpu().numpy()
    assert np.array_equal(got, _run(im, aug))                                       # the debug output changes nothing
    return pre.cpu().numpy().astype(np.float64), got


@pytest.mark.gpu
def test_noise_matches_the_float64_restatement_outside_the_band(hip):
    worst = 0.0
    for shape, cases in ((SMALL, NOISE_CASES), (FULL, NOISE_CASES[-1:])):
        im = _frame(shape, 1)
        for scale, seed in cases:
            aug = ImageAugment(stages=(('noise', scale),), seed=seed)
            pre, got = _pre_and_bytes(im, aug)
            v = _noise_pre(im, scale, seed)
            err = float(np.abs(pre - v).max())
            worst = max(worst, err)
            print("noise %s scale %g: max |device - float64| before rounding %.3g (T = %.3g), share in band %.3g"
                  % (shape, scale, err, T_NOISE, _band_share(v, T_NOISE)))
            _check_band(got, v, T_NOISE, "noise %s %g" % (shape, scale))
            assert err <= T_NOISE
            # every channel its own draw
            delta = got.astype(np.int64) - im
            mid = (im > 100) & (im < 150)
            assert abs(np.corrcoef(delta[..., 0][mid[..., 0] & mid[..., 1]], delta[..., 1][mid[..., 0] & mid[..., 1]])[0, 1]) < 0.05
    print("noise: worst %.3g" % worst)
    # flip folded into the read
    im = _frame(SMALL, 1)
    aug = ImageAugment(flip=True, stages=(('noise', 8.0),), seed=5)
    _check_band(_run(im, aug), _noise_pre(im[:, ::-1].copy(), 8.0, 5), T_NOISE, "flip + noise")


@pytest.mark.gpu
def test_hue_saturation_matches_the_float64_restatement_outside_the_band(hip):
    worst = 0.0
    for shape, cases in ((SMALL, HUE_SAT_CASES), (FULL, HUE_SAT_CASES[:1])):
        im = _frame(shape, 1)
        for hue, sat in cases:
            aug = ImageAugment(stages=(('hue_sat', hue, sat),))
            pre, got = _pre_and_bytes(im, aug)
            v = _hue_sat_pre(im, hue, sat)
            err = float(np.abs(pre - v).max())
            worst = max(worst, err)
            print("hue_sat %s (%d, %d): max |device - float64| before rounding %.3g (T = %.3g), share in band %.3g"
                  % (shape, hue, sat, err, T_HUE_SAT, _band_share(v, T_HUE_SAT)))
            _check_band(got, v, T_HUE_SAT, "hue_sat %s (%d, %d)" % (shape, hue, sat))
            assert err <= T_HUE_SAT
    print("hue_sat: worst %.3g" % worst)
    im = _frame(SMALL, 1)
    _assert_same(_run(im, ImageAugment(stages=(('hue_sat', 0, 0),))), im, "zero offsets")
    # channel 0 is taken as R: swapping the outer channels of the frame is NOT the same operation
    swapped = _run(np.ascontiguousarray(im[..., ::-1]), ImageAugment(stages=(('hue_sat', 5, 5),)))[..., ::-1]
    assert (swapped != _run(im, ImageAugment(stages=(('hue_sat', 5, 5),)))).mean() > 0.05


COMPOSED = [
    ImageAugment(flip=True, stages=(('gaussian', 2.5), ('noise', 10.0)), affine=Affine(1.1, 0.95, 0.03, -0.02, 0.05, 1, 17),
                 dropout=(0.04, True), seed=101),
    ImageAugment(flip=False, stages=(('noise', 6.0), ('gaussian', 1.0)), seed=102),
    ImageAugment(flip=True, stages=(('hue_sat', 5, -4), ('median', 3)), dropout=(0.02, False), seed=103),
    ImageAugment(flip=False, stages=(('median', 3), ('hue_sat', -5, 3)), affine=Affine(0.9, 1.2, -0.05, 0.05, -0.05, 0, 255), seed=104),
    ImageAugment(flip=True, stages=(('sharpen', 0.6, 1.4), ('hue_sat', 3, 5)), seed=105),
    ImageAugment(flip=False, stages=(('average', 2), ('noise', 25.0)), dropout=(0.05, True), seed=106),
    ImageAugment(flip=True, stages=(('noise', 2.0), ('average', 3)), affine=Affine(1.0, 1.0, 0.05, 0.0, 0.0, 1, 0), seed=107),
    ImageAugment(flip=False, stages=(('none',), ('average', 1)), affine=Affine(1.2, 1.2, 0.0, 0.0, 0.0, 0, 128), dropout=(0.01, False),
                 seed=108),
]


def _pieces(aug):
    """The record cut into one-step records, in execution order."""
    out = [ImageAugment(flip=True)] if aug.flip else []
    out += [ImageAugment(stages=(st,), seed=aug.seed) for st in aug.active_stages]
    if aug.affine is not None:
        out.append(ImageAugment(affine=aug.affine, seed=aug.seed))
    if aug.dropout is not None:
        out.append(ImageAugment(dropout=aug.dropout, seed=aug.seed))
    return out


@pytest.mark.gpu
def test_one_call_equals_stage_by_stage(hip):
    kinds = {st[0] for a in COMPOSED for st in a.stages} | {"affine%d" % a.affine.order for a in COMPOSED if a.affine} | \
            {"dropout%d" % a.dropout[1] for a in COMPOSED if a.dropout}
    assert kinds >= {'gaussian', 'average', 'median', 'sharpen', 'noise', 'hue_sat', 'affine0', 'affine1', 'dropout0', 'dropout1'}
    assert {a.flip for a in COMPOSED} == {True, False}
    im = _frame(SMALL, 3)
    for n, aug in enumerate(COMPOSED):
        step = im
        for piece in _pieces(aug):
            step = _run(step, piece)
        whole = _run(im, aug)
        _assert_same(whole, step, "record %d" % n)
        assert (whole != im).any()
        # caller-owned buffers, a second identical call, and the seed from device memory
        dev = torch.from_numpy(im).to(DEV)
        out = torch.zeros_like(dev)
        scratch = torch.zeros(hip.frcnn_image_augment_ws_bytes(*SMALL), dtype=torch.uint8, device=DEV)
        assert ops.image_augment(dev, aug, out=out, scratch=scratch) is out
        _assert_same(out.cpu().numpy(), whole, "record %d with caller buffers" % n)
        moved = copy.copy(aug)
        moved.seed = aug.seed - 40
        word = torch.tensor([40], dtype=torch.int32, device=DEV)
        _assert_same(ops.image_augment(dev, moved, seed_dev=word).cpu().numpy(), whole, "record %d seed_dev" % n)
    # another seed: other noise, other mask
    other = copy.copy(COMPOSED[0])
    other.seed = 999
    assert (_run(im, other) != _run(im, COMPOSED[0])).mean() > 0.5
    # aliasing is rejected, as the header says
    dev = torch.from_numpy(im).to(DEV)
    with pytest.raises(_hip.HipError, match="overlap"):
        ops.image_augment(dev, COMPOSED[0], out=dev)
    big = torch.empty(hip.frcnn_image_augment_ws_bytes(*SMALL), dtype=torch.uint8, device=DEV)
    out = big[:dev.numel()].view(dev.shape)
    with pytest.raises(_hip.HipError, match="overlap"):
        ops.image_augment(dev, COMPOSED[0], out=out, scratch=big)
    with pytest.raises(_hip.HipError, match="scratch too small"):
        ops.image_augment(dev, COMPOSED[0], out=out, scratch=torch.empty(100, dtype=torch.uint8, device=DEV))
    assert torch.equal(dev.cpu(), torch.from_numpy(im))


@pytest.mark.gpu
def test_full_frame_worst_case_record(hip):
    """1280 x 1920, flip + Gaussian 9 taps + affine bilinear + per-channel dropout in one call against the restatement."""
    aug = ImageAugment(flip=True, stages=(('gaussian', 2.5),), affine=Affine(1.1, 0.95, 0.03, -0.02, 0.05, 1, 17),
                       dropout=(0.04, True), seed=77)
    im = _frame(FULL, 4)
    _assert_same(_run(im, aug), _restate(im, aug), "full frame")


def _seed_with(pred, width, height, start=0):
    for s in range(start, start + 4000):
        if pred(draw_image_augmentation(width, height, np.random.default_rng(s))):
            return s
    raise AssertionError("no generator seed found")


def _exact_only(a):
    return all(st[0] not in ('noise', 'hue_sat') for st in a.stages)


@pytest.mark.gpu
def test_get_minibatch_augments_frame_and_boxes(hip, tmp_path, monkeypatch):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import minibatch
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.layer import RoIDataLayer
    from faster_rcnn_pytorch_multimodal_amd.utils.blob import prep_im_for_blob
    cfg = C.cfg
    cfg.TRAIN.SCALES = (1.5,)
    h, w = SMALL
    im = _frame(SMALL, 6)
    path = str(tmp_path / "frame.npy")
    np.save(path, im)
    entry = _entry(path)
    plain = minibatch.get_minibatch([entry], 2, False, 0)
    # nothing else moved: augment_en=False is prep_im_for_blob of the file's pixels, byte for byte
    direct = prep_im_for_blob(im, cfg.PIXEL_MEANS, cfg.PIXEL_STDDEVS, cfg.PIXEL_ARRANGE, 1.5, device=DEV)
    assert torch.equal(plain['data'], direct.unsqueeze(0)) and plain['flipped'] is False
    np.testing.assert_array_equal(plain['gt_boxes'][:, :4], entry['boxes'] * np.float32(1.5))
    with pytest.raises(NotImplementedError, match="EN_AUG"):
        minibatch.get_minibatch([entry], 2, True, 0)
    cfg.IMAGE.EN_AUG = True
    seen = set()
    preds = (lambda a: a.flip and a.active_stages and _exact_only(a) and a.affine is None,
             lambda a: not a.flip and a.affine is not None and a.affine.order == 1 and _exact_only(a),
             lambda a: a.flip and a.affine is not None and a.dropout is not None and _exact_only(a),
             lambda a: len(a.active_stages) == 2 and not a.flip)                 # holds noise or hue / saturation
    for pred in preds:
        seed = _seed_with(pred, w, h)
        aug = draw_image_augmentation(w, h, np.random.default_rng(seed))
        before = copy.deepcopy(entry)
        blobs = []
        for _ in range(2):                                                          # the same generator state twice
            IA.set_augmentation_rng(np.random.default_rng(seed))
            blobs.append(minibatch.get_minibatch([entry], 2, True, 0))
        blob = blobs[0]
        assert torch.equal(blobs[0]['data'], blobs[1]['data']) and np.array_equal(blobs[0]['gt_boxes'], blobs[1]['gt_boxes'])
        np.testing.assert_array_equal(entry['boxes'], before['boxes'])              # the roidb itself is not modified
        np.testing.assert_array_equal(entry['ignore'], before['ignore'])
        assert blob['data'].shape == plain['data'].shape and blob['data'].is_cuda
        np.testing.assert_array_equal(blob['info'], plain['info'])
        assert blob['flipped'] is aug.flip and blob['filename'] == path
        seen.add(aug.flip)
        want = augment_image_gt_boxes(copy.deepcopy(entry), aug, w, h)
        inds = np.where(np.asarray(want['ignore']) == 0)[0]
        gt = np.empty((len(inds), 5), np.float32)
        gt[:, :4] = want['boxes'][inds] * np.float32(1.5)
        gt[:, 4] = want['gt_classes'][inds]
        np.testing.assert_array_equal(blob['gt_boxes'], gt)
        assert not torch.equal(blob['data'], plain['data'])
        frame = _restate(im, aug)
        ref = prep_im_for_blob(frame, cfg.PIXEL_MEANS, cfg.PIXEL_STDDEVS, cfg.PIXEL_ARRANGE, 1.5, device=DEV).unsqueeze(0)
        if _exact_only(aug):
            assert torch.equal(blob['data'], ref)
        else:       # a handful of samples inside the band may round the other way and spread through the later stage
            dev_frame = _run(im, aug)
            assert (dev_frame != frame).mean() < 0.01
            assert torch.equal(blob['data'], prep_im_for_blob(dev_frame, cfg.PIXEL_MEANS, cfg.PIXEL_STDDEVS, cfg.PIXEL_ARRANGE,
                                                              1.5, device=DEV).unsqueeze(0))
    assert seen == {True, False}
    # an identity draw launches nothing and returns the plain blob
    seed = _seed_with(lambda a: a.identity, w, h)

    def boom(*a, **k):
        raise AssertionError("ops.image_augment called for an identity record")

    monkeypatch.setattr(ops, "image_augment", boom)
    IA.set_augmentation_rng(np.random.default_rng(seed))
    infos, data, local = minibatch._get_image_blob([entry], 1.5, augment_en=True)
    assert torch.equal(data, plain['data']) and local[0]['flipped'] is False
    monkeypatch.undo()
    # a frame whose boxes all become ignored yields None, and the data layer moves on to the next frame
    thin = _entry(path, boxes=[[10.0, 10.0, 60.0, 11.0], [30.0, 40.0, 31.5, 90.0]])
    IA.set_augmentation_rng(np.random.default_rng(3))
    assert minibatch.get_minibatch([thin], 2, True, 0) is None
    assert minibatch.get_minibatch([thin], 2, False, 0) is not None                 # only the augmented path applies the rules
    other = str(tmp_path / "other.npy")
    np.save(other, im)
    layer = RoIDataLayer([thin, _entry(other), thin], 2, 'train')
    IA.set_augmentation_rng(np.random.default_rng(4))
    for _ in range(3):
        assert layer.forward(True)['filename'] == other


@pytest.mark.gpu
def test_image_train_net_on_augmented_frames(hip, tmp_path):
    """``train_net(imagenet(...), db, ..., augment_en=True)`` with cfg.IMAGE.EN_AUG on: the shape of
    tests/test_reference_names.py::test_train_net_entry_point_on_a_roidb with the data layer augmenting."""
    from faster_rcnn_pytorch_multimodal_amd.model.config import get_output_dir, get_output_tb_dir
    from faster_rcnn_pytorch_multimodal_amd.model.train_val import train_net
    from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
    from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
    cfg = C.cfg
    cfg.ROOT_DIR = str(tmp_path)
    cfg.TRAIN.SNAPSHOT_ITERS = 1000
    cfg.TRAIN.LEARNING_RATE = 1e-5
    cfg.IMAGE.EN_AUG = True
    cfg.TRAIN.GRAPHS = False              # eager steps: what is under test here is the data layer feeding the step
    rng = np.random.default_rng(3)
    roidb = []
    for i in range(3):
        path = str(tmp_path / ("train_%d.npy" % i))
        np.save(path, rng.integers(0, 256, (128, 192, 3), dtype=np.uint8))
        x1, y1 = rng.uniform(5, 60, 2)
        roidb.append({"filename": path, "boxes": np.array([[x1, y1, x1 + 70, y1 + 50], [100, 20, 180, 110]], np.float32),
                      "gt_classes": np.array([1, 1]), "ignore": np.array([0, 1 if i == 0 else 0]),
                      "boxes_dc": np.zeros((0, 4), np.float32), "flipped": False})

    class Db:
        name = "synthetic_train_augmented"
        num_classes = 2
        val_roidb = None

    db = Db()
    db.roidb = roidb
    net = imagenet(num_layers=101)
    net.create_architecture(db.num_classes, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    net.load_state_dict(seeded_state_dict(net, 7, bn_mode="tame"))
    w0 = net.rpn_net.weight.detach().clone()
    IA.set_augmentation_rng(np.random.default_rng(_seed_with(lambda a: not a.identity, 192, 128)))
    out_dir, tb_dir = get_output_dir(db, mode='train'), get_output_tb_dir(db, None)
    sw = train_net(net, db, out_dir, tb_dir, pretrained_model=None, max_iters=4, sum_size=2, val_sum_size=1000,
                   batch_size=2, val_batch_size=1, val_thresh=0.1, augment_en=True, val_augment_en=False)
    assert len(sw.losses) == 4 and all(np.isfinite(v) and v > 0 for v in sw.losses), sw.losses
    assert not torch.equal(net.rpn_net.weight.detach().cpu(), w0.cpu())              # the optimizer stepped
    for e in roidb:                                                                  # the roidb itself is never modified
        assert e['flipped'] is False and e['boxes'][1].tolist() == [100, 20, 180, 110]
