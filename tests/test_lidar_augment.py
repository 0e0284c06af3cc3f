"""LiDAR point-cloud augmentation and rain simulation (lib/roi_data_layer/minibatch.py:274-428): the decisions and the
gt-box side on the host (``roi_data_layer/lidar_augment.py``), the per-point transforms on the device
(``frcnn_lidar_augment``) against a numpy restatement of the reference kept in this file.  The restatement keeps every row
and a keep mask (draws are indexed by the row of the input, csrc/rng.h) and is evaluated in float32 where the device
result must be bit-equal and in float64 where a bound is asserted; the draws are replayed with the oracle's
``uniform01 / normal01``.
"""
import copy
import math

import numpy as np
import pytest
import torch

from faster_rcnn_pytorch_multimodal_amd import _hip, ops
from faster_rcnn_pytorch_multimodal_amd.model import config as C
from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_augment as LA
from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.lidar_augment import (LidarAugment, augment_gt_boxes,
                                                                             draw_lidar_augmentation)
from oracle import frcnn_oracle as O

DEV = "cuda:0"
X_RANGE, Y_RANGE, Z_RANGE = [0, 70], [-40, 40], [-3, 3]                     # cfg.LIDAR defaults = the oracle's constants
EXTENTS = [X_RANGE[0], Y_RANGE[0], Z_RANGE[0], X_RANGE[1], Y_RANGE[1], Z_RANGE[1]]
STREAM = ops.AUG_STREAM


@pytest.fixture(autouse=True)
def _fresh_cfg():
    C.reset_cfg()
    C.cfg.NET_TYPE = "lidar"
    LA.set_augmentation_rng(None)
    yield
    LA.set_augmentation_rng(None)
    C.reset_cfg()


# ---------------------------------------------------------------------------------------------------------------
# the reference, restated
# ---------------------------------------------------------------------------------------------------------------
def _point_cloud(n, seed, dense=4000):
    """Like tests/test_gpu_parity.py::_point_cloud: points beyond every range face, on the faces, voxels with > 32 points."""
    rng = np.random.default_rng(seed)
    dense = min(dense, n // 5)
    pts = np.stack((rng.uniform(-2, 72, n), rng.uniform(-42, 42, n), rng.uniform(-3.2, 3.2, n), rng.uniform(0, 3, n),
                    rng.uniform(0, 2, n)), 1).astype(np.float32)
    pts[:dense, :3] = rng.normal([10, 0, -1], [0.08, 0.08, 0.3], (dense, 3))
    pts[dense:dense + 50, 0] = 70.0
    pts[dense + 50:dense + 100, 2] = -3.0
    pts[dense + 100:dense + 120, 0] = -1.0         # outside: must not be flipped / swapped into the grid
    return pts[rng.permutation(n)]


def _in_range(x, y, z):
    return ((x >= X_RANGE[0]) & (y >= Y_RANGE[0]) & (z >= Z_RANGE[0]) & (x < X_RANGE[1]) & (y < Y_RANGE[1]) & (z < Z_RANGE[1]))


def _restate(pts, aug, dt):
    """minibatch.py:274-428 on float32 rows ``pts`` in arithmetic of type ``dt``.  Returns (rows (N, F) of type dt with
    x, y, z, intensity transformed, keep mask (N,), extras dict).  dt = float32: constants rounded to float32 first and
    one rounding per operation, i.e. what the device evaluates; dt = float64: the reference's own double arithmetic."""
    n = pts.shape[0]
    idx = np.arange(n)
    out = pts.astype(dt).copy()
    x, y, z, w = (out[:, k].copy() for k in range(4))
    keep = _in_range(pts[:, 0], pts[:, 1], pts[:, 2])                               # :274 filter_points on the raw cloud
    extra = {}
    if aug.gauss is not None:                                                       # :309-319
        for k, (name, v) in enumerate(zip(("gauss_x", "gauss_y", "gauss_z"), (x, y, z))):
            v += dt(aug.gauss[k]) * O.normal01(aug.seed, STREAM[name], idx).astype(dt)
    if aug.p_keep is not None:                                                      # :321-325
        keep &= O.uniform01(aug.seed, STREAM["dropout"], idx) < np.float32(aug.p_keep)
    if aug.rotation is not None:                                                    # :330-349, :695-714
        c, s = dt(math.cos(aug.rotation)), dt(math.sin(aug.rotation))
        x, y = c * x - s * y, s * x + c * y
    if aug.swap_xy:                                                                 # :351-373
        x, y = y - dt(Y_RANGE[0]), x - dt((X_RANGE[1] - X_RANGE[0]) / 2.0)
    if aug.flip_y:                                                                  # :375-384
        y = -y
    if aug.flip_x:                                                                  # :386-395
        x = -x + dt(X_RANGE[1])
    if aug.rain_rate is not None:                                                   # :397-421
        assert dt is np.float64
        r = np.sqrt(x * x + y * y + z * z)
        z_max = aug.rain_max_range
        rho = 0.9 / np.pi
        big_r = np.power(aug.rain_rate, 0.6)
        p_min = rho / (np.pi * z_max * z_max)
        sigma = 0.02 * r * np.power(1 - np.exp(-aug.rain_rate), 2)
        shift = sigma * O.normal01(aug.seed, STREAM["rain"], idx).astype(np.float64)
        r = r + shift
        x, y, z = x + shift / 3.0, y + shift / 3.0, z + shift / 3.0
        delta = np.exp(-2 * 0.01 * big_r * r)
        p_n = (rho / (r * r + np.finfo(np.float64).eps)) * delta
        w = w * delta
        extra.update(sigma=sigma, ratio=p_n / p_min, before_rain=keep.copy())
        keep &= p_n >= p_min
    if aug.test_dropout:                                                            # :422-425
        keep &= O.uniform01(aug.seed, STREAM["test_dropout"], idx) < np.float32(0.8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = x, y, z, w
    return out, keep, extra


def _max_points_per_voxel(rows, scale):
    """Largest number of in-range points sharing one voxel (the first-32-points rule needs > 32 somewhere)."""
    rows = rows[_in_range(rows[:, 0], rows[:, 1], rows[:, 2])].astype(np.float64)
    size = np.array([0.1 / scale, 0.1 / scale, 0.5])
    cells = np.floor((rows[:, :3] - np.array([X_RANGE[0], Y_RANGE[0], Z_RANGE[0]])) / size).astype(np.int64)
    return int(np.unique(cells, axis=0, return_counts=True)[1].max())


def _final_count(rows, keep):
    return int((keep & _in_range(rows[:, 0], rows[:, 1], rows[:, 2])).sum())        # :426 second filter_points


def _restate_boxes(entry, aug):
    """The gt side of minibatch.py:330-395, copied statement by statement onto one roidb entry."""
    e = copy.deepcopy(entry)
    e['flipped'] = False
    rng_ok = lambda b: bool((b[0] >= X_RANGE[0]) & (b[1] >= Y_RANGE[0]) & (b[2] >= Z_RANGE[0]) &
                            (b[0] < X_RANGE[1]) & (b[1] < Y_RANGE[1]) & (b[2] < Z_RANGE[1]))
    if aug.rotation is not None:
        gt = e['boxes']
        cosa, sina = np.cos(aug.rotation), np.sin(aug.rotation)
        rot = np.array([[cosa, sina, 0.0], [-sina, cosa, 0.0], [0.0, 0.0, 1.0]])
        gt[:, 0:3] = np.matmul(gt[:, 0:3], rot)
        gt[:, 6] += aug.rotation
        for k, b in enumerate(gt):
            e['ignore'][k] = True
            if rng_ok(b):
                e['ignore'][k] = False
    if aug.swap_xy:
        gt = e['boxes']
        x_range_mean = (X_RANGE[1] - X_RANGE[0]) / 2.0
        gx, gy = np.copy(gt[:, 0]), np.copy(gt[:, 1])
        gt[:, 0] = gy - Y_RANGE[0]
        gt[:, 1] = gx - x_range_mean
        gt[:, 6] = -gt[:, 6] + np.pi / 2.0
        for k, b in enumerate(gt):
            e['ignore'][k] = True
            if rng_ok(b):
                e['ignore'][k] = False
    if aug.flip_y:
        e['flipped'] = True
        old_y, old_ry = e['boxes'][:, 1].copy(), e['boxes'][:, 6].copy()
        y_mean = (Y_RANGE[0] + Y_RANGE[1]) / 2
        e['boxes'][:, 1] = -(old_y - y_mean) + y_mean
        e['boxes'][:, 6] = -old_ry
    if aug.flip_x:
        e['flipped'] = True
        old_x, old_ry = e['boxes'][:, 0].copy(), e['boxes'][:, 6].copy()
        x_mean = (X_RANGE[0] + X_RANGE[1]) / 2
        e['boxes'][:, 0] = -(old_x - x_mean) + x_mean
        e['boxes'][:, 6] = -old_ry
    return e


def _entry(filename="frame.npy"):
    boxes = np.array([[12.0, 3.0, -1.0, 4.7, 2.1, 1.8, 0.3],
                      [40.0, -20.0, -0.5, 4.2, 1.9, 1.6, -1.2],
                      [66.0, 35.0, 0.2, 4.9, 2.2, 1.7, 2.0],          # a corner: rotated / swapped out of range
                      [5.0, -38.0, -2.0, 3.9, 1.7, 1.5, 0.0],
                      [30.0, 10.0, -1.2, 4.5, 2.0, 1.6, 1.0]], dtype=np.float64)
    return {"filename": filename, "boxes": boxes, "gt_classes": np.array([1, 1, 1, 1, 1]),
            "ignore": np.array([0, 0, 0, 0, 1]), "boxes_dc": np.zeros((0, 7)), "flipped": False}


BOX_CASES = {
    "flip_x": LidarAugment(flip_x=True), "flip_y": LidarAugment(flip_y=True), "swap": LidarAugment(swap_xy=True),
    "rotate": LidarAugment(rotation=0.9), "rotate_neg": LidarAugment(rotation=-1.3),
    "gauss_dropout": LidarAugment(gauss=(0.05, 0.03, 0.02), p_keep=0.9, seed=5),
    "all": LidarAugment(flip_x=True, flip_y=True, swap_xy=True, rotation=0.6, gauss=(0.01, 0.02, 0.03), p_keep=0.85, seed=9),
}


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(BOX_CASES))
def test_augment_gt_boxes_matches_the_reference(case):
    aug = BOX_CASES[case]
    want = _restate_boxes(_entry(), aug)
    entry = _entry()
    got = augment_gt_boxes(entry, aug)
    assert got is entry
    np.testing.assert_array_equal(got['boxes'], want['boxes'])
    np.testing.assert_array_equal(np.asarray(got['ignore']), np.asarray(want['ignore']))
    assert got['flipped'] is want['flipped'] and got['flipped'] == (aug.flip_x or aug.flip_y)
    np.testing.assert_array_equal(got['boxes'][:, 3:6], _entry()['boxes'][:, 3:6])       # l, w, h never change
    if case in ("rotate", "swap", "all"):
        assert np.asarray(want['ignore']).any() and not np.asarray(want['ignore']).all()  # some box left the range
    if case in ("rotate", "swap"):                # the flags are RECOMPUTED: the box ignored in the roidb counts again when in range
        assert bool(want['ignore'][4]) == (not _in_box_range(want['boxes'][4]))
    if case == "gauss_dropout":
        np.testing.assert_array_equal(got['boxes'], _entry()['boxes'])
        np.testing.assert_array_equal(got['ignore'], _entry()['ignore'])


def _in_box_range(b):
    return bool(_in_range(b[0], b[1], b[2]))


def test_draw_is_repeatable_and_follows_the_reference_distribution():
    a = [draw_lidar_augmentation(np.random.default_rng(11)) for _ in range(2)]
    assert a[0] == a[1]
    C.cfg.LIDAR.EN_AUG_ROTATE = True
    rng = np.random.default_rng(2024)
    n = 4000
    draws = [draw_lidar_augmentation(rng) for _ in range(n)]
    assert draws != [draw_lidar_augmentation(np.random.default_rng(1)) for _ in range(n)]
    freq = {"flip_x": (np.mean([d.flip_x for d in draws]), 0.5), "flip_y": (np.mean([d.flip_y for d in draws]), 0.5),
            "gauss": (np.mean([d.gauss is not None for d in draws]), 0.3),
            "dropout": (np.mean([d.p_keep is not None for d in draws]), 0.3),
            "rotate": (np.mean([d.rotation is not None for d in draws]), 0.3),
            "swap": (np.mean([d.swap_xy for d in draws]), 0.3)}
    for name, (f, p) in freq.items():
        assert abs(f - p) <= 4 * math.sqrt(p * (1 - p) / n), (name, f, p)
    for d in draws:
        if d.gauss is not None:
            assert 0 <= d.gauss[0] <= 0.07 and 0 <= d.gauss[1] <= 0.07 and 0 <= d.gauss[2] <= 0.05
        if d.p_keep is not None:
            assert 0.8 <= d.p_keep <= 1.0
        if d.rotation is not None:
            assert -np.pi / 2 <= d.rotation <= np.pi / 2
        assert d.rain_rate is None and not d.test_dropout and 0 <= d.seed < 2 ** 32
    # the two flips are independent draws
    both = np.mean([d.flip_x and d.flip_y for d in draws])
    assert abs(both - 0.25) <= 4 * math.sqrt(0.25 * 0.75 / n)
    # rng=None: the generator installed for the run, else fresh entropy
    LA.set_augmentation_rng(np.random.default_rng(5))
    first = draw_lidar_augmentation()
    LA.set_augmentation_rng(np.random.default_rng(5))
    assert draw_lidar_augmentation() == first
    LA.set_augmentation_rng(None)
    assert len({draw_lidar_augmentation().seed for _ in range(8)}) > 1


def test_draw_with_every_switch_off_is_the_identity():
    for key in ("EN_AUG_FLIPS", "EN_AUG_GAUSS_DISTORT", "EN_AUG_DROPOUT", "EN_AUG_ROTATE", "EN_AUG_SWAP_X_Y"):
        C.cfg.LIDAR[key] = False
    rng = np.random.default_rng(0)
    for _ in range(50):
        d = draw_lidar_augmentation(rng)
        assert d == LidarAugment() and d.identity
    assert draw_lidar_augmentation(rng, augment_en=False, mode='test') == LidarAugment()
    C.reset_cfg()
    assert draw_lidar_augmentation(rng, augment_en=False) == LidarAugment()               # train mode, augment_en off
    # only the enabled switches draw (EN_AUG_ROTATE is off by default)
    assert all(draw_lidar_augmentation(rng).rotation is None for _ in range(200))
    # test-time switches
    C.cfg.TEST.DROPOUT_EN = True
    d = draw_lidar_augmentation(rng, augment_en=False, mode='test')
    assert d.test_dropout and d.rain_rate is None and not d.identity
    assert draw_lidar_augmentation(rng, augment_en=False, mode='train').identity           # train mode ignores them
    C.cfg.TEST.RAIN_SIM_EN = True
    with pytest.raises(ValueError, match="LIDAR_MAX_RANGE"):
        draw_lidar_augmentation(rng, augment_en=False, mode='test')
    for name, rmax in (("waymo", 200.0), ("kitti", 120.0), ("cadc", 200.0)):
        C.cfg.DB_NAME = name
        d = draw_lidar_augmentation(rng, augment_en=False, mode='test')
        assert d.rain_rate == 1.0 and d.rain_max_range == rmax and d.test_dropout


def test_config_keys_have_the_reference_defaults():
    cfg = C.cfg
    assert (cfg.LIDAR.EN_AUG_FLIPS, cfg.LIDAR.EN_AUG_GAUSS_DISTORT, cfg.LIDAR.EN_AUG_DROPOUT, cfg.LIDAR.EN_AUG_ROTATE,
            cfg.LIDAR.EN_AUG_SWAP_X_Y, cfg.LIDAR.SHUFFLE_PC) == (True, True, True, False, True, False)
    assert (cfg.TEST.RAIN_SIM_EN, cfg.TEST.DROPOUT_EN, cfg.TEST.RAIN_RATE) == (False, False, 1)
    assert (cfg.WAYMO.LIDAR_MAX_RANGE, cfg.KITTI.LIDAR_MAX_RANGE, cfg.CADC.LIDAR_MAX_RANGE) == (200, 120, 200)
    C.cfg_from_list(["LIDAR.EN_AUG_ROTATE", "True", "LIDAR.EN_AUG_FLIPS", "False", "TEST.RAIN_SIM_EN", "True",
                     "TEST.RAIN_RATE", "30", "TEST.DROPOUT_EN", "True", "KITTI.LIDAR_MAX_RANGE", "100"])
    assert cfg.LIDAR.EN_AUG_ROTATE is True and cfg.LIDAR.EN_AUG_FLIPS is False and cfg.TEST.RAIN_SIM_EN is True
    assert cfg.TEST.RAIN_RATE == 30 and cfg.TEST.DROPOUT_EN is True and cfg.KITTI.LIDAR_MAX_RANGE == 100
    C.reset_cfg()
    assert C.cfg.TEST.RAIN_RATE == 1 and C.cfg.LIDAR.EN_AUG_ROTATE is False


def test_lidar_augment_argument_errors_are_reported_without_a_gpu():
    lib = _hip.load()
    assert lib.frcnn_version() >= 110
    rng_, par = _hip.float_array(EXTENTS), _hip.float_array([0, 0, 0, 1.0, 1, 0, 0, 0])
    fake = 4096                                                  # a non-null device address: never dereferenced on the host

    def call(points=fake, n=100, stride=4, rng=rng_, flags=0, params=par, out=fake, kept=fake, max_blocks=0):
        return lib.frcnn_lidar_augment(points, n, stride, rng, flags, params, 1, None, out, kept, max_blocks, None)

    for kw in (dict(points=None), dict(out=None), dict(kept=None), dict(rng=None), dict(params=None)):
        assert call(**kw) == -1 and b"null" in lib.frcnn_last_error(), kw
    assert call(stride=3) == -1 and b"4 floats" in lib.frcnn_last_error()
    assert call(n=0) == -1 and call(n=-5) == -1 and b"num_points" in lib.frcnn_last_error()
    for bad in (0.0, -0.1, 1.5, float("nan")):
        assert call(params=_hip.float_array([0, 0, 0, bad, 1, 0, 0, 0])) == -1, bad
        assert b"p_keep" in lib.frcnn_last_error()
    assert call(flags=1 << 9) == -1 and b"flag" in lib.frcnn_last_error()
    assert call(flags=ops.AUG_RAIN) == -1 and b"rain" in lib.frcnn_last_error()            # rate / max range missing
    assert call(out=fake + 16) == -1 and b"overlap" in lib.frcnn_last_error()
    assert call(max_blocks=-1) == -1
    assert call(rng=_hip.float_array([0, 0, 0, 0, 1, 1])) == -1 and b"range" in lib.frcnn_last_error()
    with pytest.raises(_hip.HipError, match="no CPU path"):
        ops.lidar_augment_points(torch.zeros(10, 4), LidarAugment(flip_x=True), 1, EXTENTS)


def test_unsupported_switches_raise(tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import minibatch
    path = str(tmp_path / "cloud.npy")
    np.save(path, _point_cloud(200, 1))
    C.cfg.LIDAR.SHUFFLE_PC = True
    with pytest.raises(NotImplementedError, match="SHUFFLE_PC"):
        minibatch._get_lidar_blob([path], EXTENTS, 0.5, augment_en=False, mode='test', device='cpu')
    C.cfg.LIDAR.SHUFFLE_PC = False
    with pytest.raises(NotImplementedError, match="mode='test'"):
        minibatch._get_lidar_blob([path], EXTENTS, 0.5, augment_en=True, mode='test', device='cpu')
    C.cfg.TEST.RAIN_SIM_EN = True
    with pytest.raises(ValueError, match="LIDAR_MAX_RANGE"):
        minibatch._get_lidar_blob([path], EXTENTS, 0.5, augment_en=False, mode='test', device='cpu')


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def _run(pts, aug, **kw):
    dev = torch.from_numpy(pts).to(DEV)
    out, kept = ops.lidar_augment_points(dev, aug, aug.seed, EXTENTS, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), torch.from_numpy(pts)) or kw.get("out") is dev            # the input is not touched
    return out, out.cpu().numpy(), int(kept.item())


def _check_rows(got, pts, keep):
    """Dropped rows: x, y, z NaN; every column the kernel does not transform is carried over."""
    assert np.isnan(got[~keep, :3]).all() and not np.isnan(got[keep, :3]).any()
    np.testing.assert_array_equal(got[:, 4:], pts[:, 4:])


def _assert_bev_matches(dev_points, ref_rows, scale, max_voxels, elong):
    """Exactly the assertions of tests/test_gpu_parity.py::test_bev_voxelize_matches_oracle."""
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.minibatch import get_lidar_blob
    C.cfg.LIDAR.MAX_NUM_VOXEL = max_voxels
    info_ref, ref = O.get_lidar_blob(ref_rows, scale, elongation=elong is not None, max_voxels=max_voxels)
    infos, blob = get_lidar_blob(dev_points, scale, device=DEV, elongation=elong)
    got = blob.cpu().numpy()
    assert got.shape == ref.shape and infos[0] == info_ref.tolist()
    np.testing.assert_array_equal(got != 0, ref != 0)
    np.testing.assert_array_equal(got[..., :13], ref[..., :13])
    np.testing.assert_allclose(got[..., 13:], ref[..., 13:], rtol=2e-6, atol=1e-7)
    if elong is None:
        assert (got[..., 14] == 0).all()
    return ref


EXACT_CASES = {
    "prefilter": LidarAugment(seed=1),
    "flip_x": LidarAugment(flip_x=True), "flip_y": LidarAugment(flip_y=True), "swap": LidarAugment(swap_xy=True),
    "flip_xy": LidarAugment(flip_x=True, flip_y=True), "swap_flip_x": LidarAugment(swap_xy=True, flip_x=True),
    "swap_flip_xy": LidarAugment(swap_xy=True, flip_x=True, flip_y=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [4, 5])
@pytest.mark.parametrize("case", sorted(EXACT_CASES))
def test_exact_steps_are_bit_equal(hip, case, cols):
    """Pre-filter, flips and the swap round once per operation: device rows == float32 restatement bit for bit, dropped
    rows NaN, kept_count equal; and the BEV blob made from the device rows == the oracle's blob of the compacted
    restated rows (the NaN-row convention is the reference's order-preserving compaction)."""
    aug = EXACT_CASES[case]
    pts = np.ascontiguousarray(_point_cloud(30000, seed=len(case) + cols)[:, :cols])
    want, keep, _ = _restate(pts, aug, np.float32)
    assert want.dtype == np.float32 and 0 < keep.sum() < len(keep)
    dev, got, kept = _run(pts, aug)
    _check_rows(got, pts, keep)
    np.testing.assert_array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32))
    assert kept == _final_count(want, keep)
    if case != "prefilter":
        assert not np.array_equal(got[keep, :2], pts[keep, :2])
    elong = 4 if cols == 5 else None
    _assert_bev_matches(dev, want[keep], 0.5, 25000, elong)
    assert _max_points_per_voxel(want[keep], 0.5) > 32                              # the > 32 points rule is exercised


@pytest.mark.gpu
@pytest.mark.parametrize("angle", [0.0, 0.7, -1.5, np.pi / 2, -np.pi / 2])
def test_rotation_against_float64(hip, angle):
    """x' = c x - s y, y' = s x + c y with c, s rounded to float32 (relative error e1 <= 2^-24 = u), each product rounded
    (e2), the sum rounded (e3): |x' - exact| <= |c x| (2u + u) + |s y| (2u + u) + O(u^2) <= 3u (|x| + |y|) because
    |c|, |s| <= 1; the second-order terms are far below the fourth u the bound 4 * 2^-24 * (|x| + |y|) leaves."""
    aug = LidarAugment(rotation=float(angle))
    pts = _point_cloud(30000, seed=77)
    want, keep, _ = _restate(pts, aug, np.float64)
    _, got, kept = _run(pts, aug)
    _check_rows(got, pts, keep)
    bound = 4 * 2.0 ** -24 * (np.abs(pts[keep, 0].astype(np.float64)) + np.abs(pts[keep, 1].astype(np.float64)))
    for k in (0, 1):
        err = np.abs(got[keep, k].astype(np.float64) - want[keep, k])
        print("rotation %.3f axis %d: worst err / bound %.3f" % (angle, k, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all()
    np.testing.assert_array_equal(got[keep, 2:], pts[keep, 2:])
    assert kept == _final_count(got, keep)                                          # counted on the device's own rows


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [4, 5])
def test_gauss_distortion_and_dropout_follow_the_replayed_draws(hip, cols):
    """|err| <= ulp(coordinate) + sigma * 2e-5 against float64 with the replayed normal01 draws (2e-5: the allowance for
    logf / cosf last-ulp differences of tests/test_uncertainty.py); the dropout keep mask is integer arithmetic: bit-equal."""
    aug = LidarAugment(gauss=(0.07, 0.05, 0.03), p_keep=0.83, seed=0xC0FFEE)
    pts = np.ascontiguousarray(_point_cloud(30000, seed=5)[:, :cols])
    want, keep, _ = _restate(pts, aug, np.float64)
    pre = _in_range(pts[:, 0], pts[:, 1], pts[:, 2])
    assert 0.80 < keep.sum() / pre.sum() < 0.86
    _, got, kept = _run(pts, aug)
    _check_rows(got, pts, keep)                                                     # includes: mask bit-equal to the replay
    for k in range(3):
        err = np.abs(got[keep, k].astype(np.float64) - want[keep, k])
        bound = np.spacing(np.abs(want[keep, k]).astype(np.float32)).astype(np.float64) + aug.gauss[k] * 2e-5
        print("gauss axis %d: worst err / bound %.3f" % (k, float((err / bound).max())))
        assert (err <= bound).all()
        moved = np.abs(got[keep, k] - pts[keep, k])
        assert moved.max() > 2 * aug.gauss[k] and moved.max() < 6.5 * aug.gauss[k]
        assert abs(float(np.std(got[keep, k].astype(np.float64) - pts[keep, k])) / aug.gauss[k] - 1) < 0.03
    np.testing.assert_array_equal(got[keep, 3:], pts[keep, 3:])
    assert kept == _final_count(got, keep)


@pytest.mark.gpu
def test_test_dropout_mask_is_bit_equal(hip):
    aug = LidarAugment(test_dropout=True, seed=321)
    pts = _point_cloud(30000, seed=6)
    want, keep, _ = _restate(pts, aug, np.float32)
    pre = _in_range(pts[:, 0], pts[:, 1], pts[:, 2])
    assert 0.78 < keep.sum() / pre.sum() < 0.82
    _, got, kept = _run(pts, aug)
    _check_rows(got, pts, keep)
    np.testing.assert_array_equal(got[keep].view(np.uint32), pts[keep].view(np.uint32))
    assert kept == int(keep.sum())
    # its draws are not the training dropout's
    _, got2, _ = _run(pts, LidarAugment(p_keep=0.8, seed=321))
    assert not np.array_equal(np.isnan(got2[:, 0]), np.isnan(got[:, 0]))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("rate", [10, 30])
def test_rain_simulation_against_float64(hip, rate, seed):
    """minibatch.py:397-421 at r_max = 200 m.  Positions within ulp(coordinate) + sigma * 2e-5 (sigma = the point's own),
    intensity rtol 1e-5, keep mask equal to the float64 one for every point whose p_n / p_min is further than 1e-3 from
    1 - and that condition excludes at most 0.1 % of the in-range points (measured on the CPU with the replayed draws:
    7-9 of ~26 000 at rate 10, 3-5 at rate 30; ~32 % / ~61 % of the points are removed)."""
    aug = LidarAugment(rain_rate=float(rate), rain_max_range=200.0, seed=1000 + seed)
    pts = _point_cloud(30000, seed=seed)
    want, keep, ex = _restate(pts, aug, np.float64)
    pre = ex["before_rain"]
    unsure = pre & (np.abs(ex["ratio"] - 1.0) <= 1e-3)
    removed = 1.0 - keep.sum() / pre.sum()
    print("rain %d seed %d: %d in range, %d near the threshold, %.1f %% removed" % (rate, seed, pre.sum(), unsure.sum(),
                                                                                 100 * removed))
    assert unsure.sum() <= 1e-3 * pre.sum()
    assert 0.2 < removed < 0.75                                                     # the mask is genuinely exercised
    _, got, kept = _run(pts, aug)
    alive = ~np.isnan(got[:, 0])
    assert np.isnan(got[~alive, :3]).all() and not np.isnan(got[alive, :3]).any()
    np.testing.assert_array_equal(alive[~unsure], keep[~unsure])
    assert not alive[~pre].any()
    both = alive & keep
    for k in range(3):
        err = np.abs(got[both, k].astype(np.float64) - want[both, k])
        bound = np.spacing(np.abs(want[both, k]).astype(np.float32)).astype(np.float64) + ex["sigma"][both] * 2e-5
        print("rain axis %d: worst err / bound %.3f" % (k, float((err / bound).max())))
        assert (err <= bound).all()
    np.testing.assert_allclose(got[both, 3].astype(np.float64), want[both, 3], rtol=1e-5, atol=0)
    assert (got[both, 3] <= pts[both, 3]).all() and (got[both, 3] < pts[both, 3]).mean() > 0.99      # attenuated
    np.testing.assert_array_equal(got[:, 4:], pts[:, 4:])
    assert kept == _final_count(got, alive)


@pytest.mark.gpu
def test_rain_at_the_default_rate_only_moves_and_attenuates(hip):
    aug = LidarAugment(rain_rate=1.0, rain_max_range=200.0, seed=4)
    pts = _point_cloud(30000, seed=4)
    want, keep, ex = _restate(pts, aug, np.float64)
    np.testing.assert_array_equal(keep, ex["before_rain"])                          # nothing inside 70 x 80 m attenuates away
    _, got, _ = _run(pts, aug)
    _check_rows(got, pts, keep)
    for k in range(3):
        err = np.abs(got[keep, k].astype(np.float64) - want[keep, k])
        assert (err <= np.spacing(np.abs(want[keep, k]).astype(np.float32)) + ex["sigma"][keep] * 2e-5).all()
    np.testing.assert_allclose(got[keep, 3].astype(np.float64), want[keep, 3], rtol=1e-5, atol=0)


MIXES = {
    "train_all": (LidarAugment(flip_x=True, flip_y=True, swap_xy=True, rotation=0.4, gauss=(0.06, 0.06, 0.04), p_keep=0.85,
                               seed=17), 25000, 5),
    "train_cap": (LidarAugment(flip_y=True, gauss=(0.03, 0.07, 0.05), p_keep=0.9, seed=18), 3000, 5),
    "test_rain": (LidarAugment(rain_rate=10.0, rain_max_range=200.0, test_dropout=True, seed=19), 3000, 4),
    # (no swap / flip x here: they move the dense cluster beyond the range the rain leaves; "train_all" has them)
    "train_and_test": (LidarAugment(flip_y=True, rotation=-0.8, gauss=(0.02, 0.02, 0.02), p_keep=0.95, rain_rate=10.0,
                                    rain_max_range=200.0, test_dropout=True, seed=20), 25000, 4),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mix", sorted(MIXES))
def test_voxeliser_reads_nan_rows_like_a_compacted_cloud(hip, mix):
    """Whatever the step mix: the BEV blob of the device rows (NaN rows in place) == the oracle's blob of the same rows
    copied to the host - the NaN-row convention against the order-dependent voxel rules (voxel numbering by first
    appearance under the 3000-voxel cap, first 32 points of a voxel)."""
    aug, max_voxels, cols = MIXES[mix]
    pts = np.ascontiguousarray(_point_cloud(30000, seed=31)[:, :cols])
    dev, got, kept = _run(pts, aug)
    alive = ~np.isnan(got[:, 0])
    assert 0 < alive.sum() < len(alive) and np.isnan(got[~alive, :3]).all()
    assert kept == _final_count(got, alive)
    elong = 4 if cols == 5 else None
    ref = _assert_bev_matches(dev, got, 0.5, max_voxels, elong)                     # the oracle's filter drops the NaN rows
    ref2 = _assert_bev_matches(dev, got[alive], 0.5, max_voxels, elong)             # ... which equals compacting them away
    np.testing.assert_array_equal(ref, ref2)
    assert _max_points_per_voxel(got[alive], 0.5) > 32                              # a voxel with > 32 points
    if max_voxels == 3000:
        assert int((ref[..., :12] != 0).sum()) <= 3000
        _, uncapped = O.get_lidar_blob(got, 0.5, elongation=elong is not None, max_voxels=25000)
        assert int((uncapped[..., :12] != 0).sum()) > 3000                          # the cap is exercised


@pytest.mark.gpu
def test_launch_is_a_pure_function_of_record_and_seed(hip):
    aug = LidarAugment(flip_x=True, gauss=(0.05, 0.05, 0.05), p_keep=0.9, rain_rate=10.0, rain_max_range=200.0,
                       test_dropout=True, seed=99)
    for cols in (4, 5):
        pts = np.ascontiguousarray(_point_cloud(30000, seed=8)[:, :cols])
        _, a, ka = _run(pts, aug)
        _, b, kb = _run(pts, aug)
        assert a.tobytes() == b.tobytes() and ka == kb
        for blocks in (1, 7, 64):                                                   # a forced different grid
            _, c, kc = _run(pts, aug, max_blocks=blocks)
            assert a.tobytes() == c.tobytes() and ka == kc
        other = copy.copy(aug)
        other.seed = 100
        _, d, _ = _run(pts, other)
        both = ~np.isnan(a[:, 0]) & ~np.isnan(d[:, 0])
        assert both.sum() > 1000 and (a[both, 0] != d[both, 0]).mean() > 0.99
        assert not np.array_equal(np.isnan(a[:, 0]), np.isnan(d[:, 0]))
        # in place == out of place; the seed may come from device memory (seed + *seed_dev)
        dev = torch.from_numpy(pts).to(DEV)
        out, kept = ops.lidar_augment_points(dev, aug, aug.seed, EXTENTS, out=dev)
        assert out is dev and dev.cpu().numpy().tobytes() == a.tobytes() and int(kept.item()) == ka
        word = torch.tensor([aug.seed - 40], dtype=torch.int32, device=DEV)
        out, kept = ops.lidar_augment_points(torch.from_numpy(pts).to(DEV), aug, 40, EXTENTS, seed_dev=word)
        assert out.cpu().numpy().tobytes() == a.tobytes() and int(kept.item()) == ka


def _write_frame(tmp_path, name, pts):
    path = str(tmp_path / name)
    np.save(path, pts)
    return path


def _seed_with(pred, start=0):
    for s in range(start, start + 2000):
        if pred(draw_lidar_augmentation(np.random.default_rng(s))):
            return s
    raise AssertionError("no generator seed found")


@pytest.mark.gpu
def test_get_minibatch_augments_points_and_boxes(hip, tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import minibatch
    from faster_rcnn_pytorch_multimodal_amd.utils.bbox import bbox_pc_to_voxel_grid
    C.cfg.TRAIN.SCALES = (0.5,)
    C.cfg.LIDAR.EN_AUG_ROTATE = True
    pts = _point_cloud(30000, seed=12)
    path = _write_frame(tmp_path, "frame.npy", pts)
    entry = _entry(path)
    plain = minibatch.get_minibatch([entry], 2, False, 0)
    assert plain['flipped'] is False
    seen_flip = seen_plain = False
    for pred in (lambda a: a.flip_x and a.swap_xy and a.gauss is not None,
                 lambda a: a.rotation is not None and a.p_keep is not None and not (a.flip_x or a.flip_y),
                 lambda a: a.flip_y and not a.flip_x and a.rotation is None and not a.swap_xy):
        seed = _seed_with(pred)
        aug = draw_lidar_augmentation(np.random.default_rng(seed))
        LA.set_augmentation_rng(np.random.default_rng(seed))
        before = copy.deepcopy(entry)
        blobs = minibatch.get_minibatch([entry], 2, True, 0)
        np.testing.assert_array_equal(entry['boxes'], before['boxes'])              # the roidb itself is not modified
        np.testing.assert_array_equal(entry['ignore'], before['ignore'])
        assert blobs['data'].shape == plain['data'].shape and blobs['data'].is_cuda
        np.testing.assert_array_equal(blobs['info'], plain['info'])
        assert blobs['filename'] == path and blobs['flipped'] is (aug.flip_x or aug.flip_y)
        seen_flip |= blobs['flipped']
        seen_plain |= not blobs['flipped']
        want = augment_gt_boxes(copy.deepcopy(entry), aug)
        inds = np.where(np.asarray(want['ignore']) == 0)[0]
        gt = np.empty((len(inds), 8), np.float32)
        gt[:, :7] = bbox_pc_to_voxel_grid(np.array(want['boxes'], dtype=np.float64)[inds], EXTENTS, blobs['info'])
        gt[:, 0:2] *= 0.5
        gt[:, 3:5] *= 0.5
        gt[:, 7] = want['gt_classes'][inds]
        np.testing.assert_array_equal(blobs['gt_boxes'], gt)
        # the blob is the voxelised device cloud of that record
        dev, _, _ = _run(pts, aug)
        _, ref = minibatch.get_lidar_blob(dev, 0.5, device=DEV, elongation=None)
        assert torch.equal(blobs['data'], ref) and not torch.equal(blobs['data'], plain['data'])
    assert seen_flip and seen_plain
    # an identity record: byte-identical to the un-augmented call
    seed = _seed_with(lambda a: a.identity)
    LA.set_augmentation_rng(np.random.default_rng(seed))
    same = minibatch.get_minibatch([entry], 2, True, 0)
    assert torch.equal(same['data'], plain['data']) and np.array_equal(same['gt_boxes'], plain['gt_boxes'])


@pytest.mark.gpu
def test_frame_without_points_is_skipped(hip, tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import minibatch
    C.cfg.TRAIN.SCALES = (0.5,)
    pts = _point_cloud(2000, seed=3)
    pts[:, 1] = 39.0                                                 # the swap sends x' = y + 40 = 79 >= 70: out of range
    path = _write_frame(tmp_path, "empty_after_swap.npy", pts)
    seed = _seed_with(lambda a: a.swap_xy and not a.flip_x and not a.flip_y and a.rotation is None)
    LA.set_augmentation_rng(np.random.default_rng(seed))
    infos, blob, local = minibatch._get_lidar_blob([_entry(path)], EXTENTS, 0.5, augment_en=True)
    assert blob is None and local[0]['filename'] == path
    LA.set_augmentation_rng(np.random.default_rng(seed))
    assert minibatch.get_minibatch([_entry(path)], 2, True, 0) is None
    assert minibatch.get_minibatch([_entry(path)], 2, False, 0) is not None


@pytest.mark.gpu
def test_test_mode_rain_and_dropout(hip, tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.model.test import _get_blobs
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import minibatch
    C.cfg.TEST.SCALES = (0.5,)
    pts = _point_cloud(30000, seed=21)
    path = _write_frame(tmp_path, "scan.npy", pts)
    infos0, plain, _ = minibatch._get_lidar_blob([path], EXTENTS, 0.5, augment_en=False, mode='test')
    _, direct = minibatch.get_lidar_blob(pts, 0.5, device=DEV)
    assert torch.equal(plain, direct)                                 # switches off: the un-augmented path, byte for byte
    C.cfg.DB_NAME = 'kitti'
    C.cfg.TEST.RAIN_SIM_EN, C.cfg.TEST.RAIN_RATE = True, 30
    LA.set_augmentation_rng(np.random.default_rng(1))
    aug = draw_lidar_augmentation(np.random.default_rng(1), augment_en=False, mode='test')
    assert aug.rain_rate == 30.0 and aug.rain_max_range == 120.0 and not aug.test_dropout
    blobs = _get_blobs([path])                                        # what test_net calls per frame
    np.testing.assert_array_equal(blobs['info'], infos0[0])
    dev, _, _ = _run(pts, aug)
    assert torch.equal(blobs['data'], minibatch.get_lidar_blob(dev, 0.5, device=DEV)[1])
    assert not torch.equal(blobs['data'], plain)
    assert int((blobs['data'][..., :12] != 0).sum()) < int((plain[..., :12] != 0).sum())      # points attenuated away
    C.cfg.TEST.RAIN_SIM_EN, C.cfg.TEST.DROPOUT_EN = False, True
    LA.set_augmentation_rng(np.random.default_rng(2))
    _, dropped, _ = minibatch._get_lidar_blob([path], EXTENTS, 0.5, augment_en=False, mode='test')
    assert not torch.equal(dropped, plain)
    # train mode ignores the test-time switches
    _, train_blob, _ = minibatch._get_lidar_blob([_entry(path)], EXTENTS, 0.5, augment_en=False, mode='train')
    assert torch.equal(train_blob, plain)


@pytest.mark.gpu
def test_lidar_train_step_on_an_augmented_frame(hip, tmp_path):
    """``train_net(lidarnet(...), db, ..., augment_en=True)``: the data layer draws, augments and skips like the reference,
    and the detector trains on what it produces."""
    from faster_rcnn_pytorch_multimodal_amd.model.config import get_output_dir, get_output_tb_dir
    from faster_rcnn_pytorch_multimodal_amd.model.train_val import train_net
    from faster_rcnn_pytorch_multimodal_amd.nets.lidarnet import lidarnet
    from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
    cfg = C.cfg
    cfg.ROOT_DIR = str(tmp_path)
    cfg.TRAIN.SCALES = (0.5,)
    cfg.TRAIN.SNAPSHOT_ITERS = 1000
    cfg.TRAIN.LEARNING_RATE = 1e-5
    cfg.TRAIN.GRAPHS = False              # eager steps: what is under test here is the data layer feeding the step
    roidb = []
    for i in range(2):
        roidb.append(_entry(_write_frame(tmp_path, "train_%d.npy" % i, _point_cloud(20000, seed=40 + i))))

    class Db:
        name = "synthetic_lidar_train"
        num_classes = 2
        val_roidb = None

    db = Db()
    db.roidb = roidb
    net = lidarnet(num_layers=101)
    net.create_architecture(2, tag='default', anchor_scales=cfg.LIDAR.ANCHOR_SCALES[0], anchor_ratios=cfg.LIDAR.ANCHOR_ANGLES)
    net.load_state_dict(seeded_state_dict(net, 7, bn_mode="tame"))
    LA.set_augmentation_rng(np.random.default_rng(_seed_with(lambda a: not a.identity)))
    out_dir, tb_dir = get_output_dir(db, mode='train'), get_output_tb_dir(db, None)
    sw = train_net(net, db, out_dir, tb_dir, pretrained_model=None, max_iters=2, sum_size=2, val_sum_size=1000,
                   batch_size=2, val_batch_size=1, val_thresh=0.1, augment_en=True, val_augment_en=False)
    assert len(sw.losses) == 2 and all(np.isfinite(v) and v > 0 for v in sw.losses), sw.losses
