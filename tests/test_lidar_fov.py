"""Camera field-of-view filter of KITTI / CADC scans (lib/roi_data_layer/minibatch.py:251-268, get_fov_flag :678-693): the
calibration side on the host (``roi_data_layer/lidar_calib.py``), the per-point side on the device as the first step of
``frcnn_lidar_augment_fov``.  tests/golden/lidar_fov.npz (tests/golden/make_golden_lidar_fov.py) pins made-up calibration
files in the real formats, points, and the float64 pixel coordinates the REFERENCE's projection code computes for them;
``get_fov_flag``'s four comparisons are restated here (``_flags``) because the reference's minibatch.py cannot be imported.

The band: one composite matrix (what this package and the device evaluate) against the reference's chained products (KITTI)
/ per-point products (CADC) differs by rounding.  Measured by the generator, numpy restatement against the reference's
output, max |du| / max(1, |u|) (and the same for v) over the stored points, which include points 1e-4 m from the camera
plane where h2 cancels:
    KITTI 3.85e-12        CADC 4.66e-12
The tests assert 4 x that figure; the generator checks that no stored point lies within that band of an image edge (the
closest one is 0.14 px away), so the reference alone decides every point.
"""
import copy
import ctypes
import os

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
EXTENTS = [0, -40, -3, 70, 40, 3]                                   # cfg.LIDAR defaults
BAND = {"kitti": 4 * 3.85e-12, "cadc": 4 * 4.66e-12}               # 4 x the measured figure (module docstring)
IMG_SIZE = {"kitti": [375, 1242], "cadc": [624, 1280]}              # lib/model/config.py:442,447  [height, width]
CASES = ["kitti_plain", "kitti_tilted", "kitti_dated", "cadc_plain", "cadc_skewed"]


@pytest.fixture(autouse=True)
def _fresh_cfg():
    C.reset_cfg()
    C.cfg.NET_TYPE = "lidar"
    LA.set_augmentation_rng(None)
    yield
    LA.set_augmentation_rng(None)
    C.reset_cfg()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "lidar_fov.npz")) as z:
        return {k: z[k] for k in z.files}


def _case(golden, name, tmp_path):
    """(db, calibration file written under tmp_path, xyz float32 (N, 3), reference pixel coordinates float64 (N, 2))."""
    path = str(tmp_path / (name + ".txt"))
    with open(path, "w") as f:
        f.write(str(golden[name + "_calib"]))
    return str(golden[name + "_db"]), path, golden[name + "_xyz"], golden[name + "_uv"]


def _flags(uv, img_size):
    """get_fov_flag (minibatch.py:689-691), restated: img_shape = [height, width]."""
    val_flag_1 = np.logical_and(uv[:, 0] >= 0, uv[:, 0] < img_size[1])
    val_flag_2 = np.logical_and(uv[:, 1] >= 0, uv[:, 1] < img_size[0])
    return np.logical_and(val_flag_1, val_flag_2)


def _project(m, xyz):
    """The arithmetic the issue sets for the device, in numpy float64: h = M [x y z 1], u = h0 / h2, v = h1 / h2."""
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.concatenate((xyz.astype(np.float64), np.ones((xyz.shape[0], 1))), 1) @ np.asarray(m, np.float64).T
        return h[:, 0:2] / h[:, 2:3], h[:, 2]


def _near_edge(uv, img_size, band):
    near = np.zeros(uv.shape[0], bool)
    for col, edges in ((0, (0.0, float(img_size[1]))), (1, (0.0, float(img_size[0])))):
        for edge in edges:
            near |= np.abs(uv[:, col] - edge) <= band * np.maximum(1.0, np.abs(uv[:, col]))
    return near


def _rows(xyz, cols, seed=0):
    """(N, cols) float32 rows: the stored coordinates plus seeded intensity (/ elongation) columns."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.concatenate((xyz, rng.uniform(0, 3, (xyz.shape[0], cols - 3)).astype(np.float32)), 1))


# ---------------------------------------------------------------------------------------------------------------
# CPU: calibration files -> M
# ---------------------------------------------------------------------------------------------------------------
def test_config_carries_the_camera_frame_sizes():
    assert list(C.cfg.KITTI.IMG_SIZE) == [375, 1242] and list(C.cfg.CADC.IMG_SIZE) == [624, 1280]
    assert (C.cfg.WAYMO.LIDAR_MAX_RANGE, C.cfg.KITTI.LIDAR_MAX_RANGE, C.cfg.CADC.LIDAR_MAX_RANGE) == (200, 120, 200)


@pytest.mark.parametrize("name", CASES)
def test_composite_matrix_against_the_reference_pixels(golden, name, tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_calib
    db, path, xyz, uv_ref = _case(golden, name, tmp_path)
    m = lidar_calib.load_projection(path, db)
    assert m.shape == (3, 4) and m.dtype == np.float64 and m.flags["C_CONTIGUOUS"]
    uv, h2 = _project(m, xyz)
    rel = np.abs(uv - uv_ref) / np.maximum(1.0, np.abs(uv_ref))
    print("%s: max rel du %.2e dv %.2e (bound %.2e), min |h2| %.1e" % (name, rel[:, 0].max(), rel[:, 1].max(), BAND[db],
                                                                    np.abs(h2).min()))
    assert (rel <= BAND[db]).all()
    # the flags: restated comparisons on this package's pixels == on the reference's pixels, on EVERY point
    want = _flags(uv_ref, IMG_SIZE[db])
    assert not _near_edge(uv_ref, IMG_SIZE[db], BAND[db]).any()                    # the reference alone decides
    np.testing.assert_array_equal(_flags(uv, IMG_SIZE[db]), want)
    np.testing.assert_array_equal(lidar_calib.fov_flags(lidar_calib.project_points(m, xyz), IMG_SIZE[db]), want)
    assert 100 < want.sum() < len(want) - 100
    assert (want & (h2 < 0)).sum() > 20                                             # points behind the camera are kept
    assert np.abs(h2).min() < 1e-3                                                  # points next to the camera plane


def test_calibration_file_names_and_the_override(golden, tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_calib
    assert lidar_calib.calib_filename("/d/kitti/training/velodyne/000123.bin", "kitti") == "/d/kitti/training/calib/000123.txt"
    assert (lidar_calib.calib_filename("/d/cadc/2019_02_27/0010/point_clouds/0000000042.bin", "cadc")
            == "/d/cadc/2019_02_27/0010/calib/0000000042.txt")
    with pytest.raises(ValueError, match="waymo"):
        lidar_calib.calib_filename("/d/x.bin", "waymo")
    # frame_projection: derived name, then the roidb entry's optional 'calib' key
    for name, scan_dir in (("kitti_plain", "velodyne"), ("cadc_plain", "point_clouds")):
        db, path, _, _ = _case(golden, name, tmp_path)
        C.cfg.DB_NAME = db
        os.makedirs(str(tmp_path / db / "calib"))
        derived = str(tmp_path / db / "calib" / "7.txt")
        with open(derived, "w") as f:
            f.write(str(golden[name + "_calib"]))
        scan = str(tmp_path / db / scan_dir / "7.bin")
        m, size = lidar_calib.frame_projection(scan, {"filename": scan})
        assert size == IMG_SIZE[db] and np.array_equal(m, lidar_calib.load_projection(path, db))
        other = "kitti_tilted" if db == "kitti" else "cadc_skewed"
        _, other_path, _, _ = _case(golden, other, tmp_path)
        m2, _ = lidar_calib.frame_projection(scan, {"filename": scan, "calib": other_path})
        assert np.array_equal(m2, lidar_calib.load_projection(other_path, db)) and not np.array_equal(m2, m)
        m3, _ = lidar_calib.frame_projection(scan)                                  # test mode: no roidb entry
        assert np.array_equal(m3, m)
        C.cfg[db.upper()].IMG_SIZE = [100, 200]
        assert lidar_calib.frame_projection(scan)[1] == [100, 200]


def test_calibration_errors(golden, tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_calib
    kitti, cadc = str(golden["kitti_plain_calib"]), str(golden["cadc_plain_calib"])

    def write(text, name="bad.txt"):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write(text)
        return path

    for key in ("P2", "R0_rect", "Tr_velo_to_cam"):
        text = "\n".join(line for line in kitti.splitlines() if not line.startswith(key + ":"))
        with pytest.raises(ValueError, match=r"bad\.txt.*%s" % key):
            lidar_calib.kitti_projection(write(text))
    short = "\n".join(line.rsplit(" ", 1)[0] if line.startswith("R0_rect:") else line for line in kitti.splitlines())
    with pytest.raises(ValueError, match=r"bad\.txt.*R0_rect"):
        lidar_calib.kitti_projection(write(short))
    # a key whose values are not floats is skipped, hence missing
    dated = "\n".join("P2: 09-Jan-2012 13:57:47" if line.startswith("P2:") else line for line in kitti.splitlines())
    with pytest.raises(ValueError, match="P2"):
        lidar_calib.kitti_projection(write(dated))
    for key in ("T_LIDAR_CAM00", "CAM00_matrix"):
        text = "\n".join(line for line in cadc.splitlines() if not line.startswith(key + ":"))
        with pytest.raises(ValueError, match=r"bad\.txt.*%s" % key):
            lidar_calib.cadc_projection(write(text))
    short = "\n".join(line.rsplit(" ", 1)[0] if line.startswith("T_LIDAR_CAM00:") else line for line in cadc.splitlines())
    with pytest.raises(ValueError, match="T_LIDAR_CAM00"):
        lidar_calib.cadc_projection(write(short))
    words = "\n".join(line.rsplit(" ", 1)[0] + " abc" if line.startswith("CAM00_matrix:") else line for line in cadc.splitlines())
    with pytest.raises(ValueError, match="CAM00_matrix"):
        lidar_calib.cadc_projection(write(words))
    singular = "\n".join("T_LIDAR_CAM00: " + " ".join(["0"] * 16) if line.startswith("T_LIDAR_CAM00:") else line
                         for line in cadc.splitlines())
    with pytest.raises(ValueError, match="singular"):
        lidar_calib.cadc_projection(write(singular))
    with pytest.raises(ValueError, match="waymo"):
        lidar_calib.load_projection(write(kitti), "waymo")


def test_cadc_matrices_are_read_as_float32(golden, tmp_path):
    """CADC_utils.py:34,36: both matrices go through float32 before the float64 inverse and product."""
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_calib
    _, path, _, _ = _case(golden, "cadc_skewed", tmp_path)
    rows = {line.split(":")[0]: line.split(":")[1].split() for line in str(golden["cadc_skewed_calib"]).splitlines()}
    k4 = np.eye(4)
    k4[:3, :3] = np.array(rows["CAM00_matrix"]).astype(np.float32).reshape(3, 3)
    t = np.array(rows["T_LIDAR_CAM00"]).astype(np.float32).reshape(4, 4)
    np.testing.assert_array_equal(lidar_calib.cadc_projection(path), np.matmul(k4, np.linalg.inv(t))[:3])
    t64 = np.array(rows["T_LIDAR_CAM00"]).astype(np.float64).reshape(4, 4)
    assert not np.array_equal(lidar_calib.cadc_projection(path), np.matmul(k4, np.linalg.inv(t64))[:3])


@pytest.mark.parametrize("db", ["kitti", "cadc", "waymo"])
def test_read_point_cloud_file_returns_the_raw_rows(tmp_path, db):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import minibatch
    C.cfg.DB_NAME = db
    pts = np.random.default_rng(1).uniform(-50, 50, (300, 4)).astype(np.float32)
    path = str(tmp_path / "scan.bin")
    pts.tofile(path)
    got = minibatch.read_point_cloud_file(path)
    assert got.dtype == np.float32 and np.array_equal(got, pts)


def test_fov_entry_argument_errors_are_reported_without_a_gpu():
    lib = _hip.load()
    assert lib.frcnn_version() >= 112
    rng_, par = _hip.float_array(EXTENTS), _hip.float_array([0, 0, 0, 1.0, 1, 0, 0, 0])
    fake = 4096                                                  # a non-null device address: never dereferenced on the host
    good = (ctypes.c_double * 12)(*range(1, 13))

    def call(points=fake, n=100, stride=4, flags=0, out=fake, kept=fake, proj=good, img_h=375, img_w=1242):
        return lib.frcnn_lidar_augment_fov(points, n, stride, rng_, flags, par, 1, None, out, kept, 0, proj, img_h, img_w, None)

    assert call(proj=None) == -1 and b"projection" in lib.frcnn_last_error()
    assert call(points=None) == -1 and b"null" in lib.frcnn_last_error()
    assert call(stride=3) == -1 and b"4 floats" in lib.frcnn_last_error()
    assert call(img_h=0) == -1 and b"image size" in lib.frcnn_last_error()
    assert call(img_w=-3) == -1 and b"image size" in lib.frcnn_last_error()
    for bad in (float("nan"), float("inf")):
        m = (ctypes.c_double * 12)(*([1.0] * 5 + [bad] + [1.0] * 6))
        assert call(proj=m) == -1 and b"entry 5" in lib.frcnn_last_error()
    assert call(flags=1 << 9) == -1 and b"flag" in lib.frcnn_last_error()
    with pytest.raises(_hip.HipError, match="no CPU path"):
        ops.lidar_fov_filter(torch.zeros(10, 4), np.eye(3, 4), [4, 8])
    with pytest.raises(_hip.HipError, match="go together"):
        ops.lidar_augment_points(torch.zeros(10, 4), LidarAugment(), 1, EXTENTS, proj=np.eye(3, 4))


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def _filter(rows, m, img_size, **kw):
    dev = torch.from_numpy(rows).to(DEV)
    out, kept = ops.lidar_fov_filter(dev, m, img_size, **kw)
    torch.cuda.synchronize()
    assert kw.get("out") is dev or dev.cpu().numpy().tobytes() == rows.tobytes()             # the input is not touched
    return out, out.cpu().numpy(), int(kept.item())


def _same_bytes(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()                  # (NaN rows: torch.equal would say no)


def _check_filtered(got, rows, alive):
    """Kept rows bit-equal to the input; rejected rows NaN in x, y, z and columns 3.. untouched."""
    np.testing.assert_array_equal(got[alive].view(np.uint32), rows[alive].view(np.uint32))
    assert np.isnan(got[~alive, :3]).all()
    np.testing.assert_array_equal(got[:, 3:].view(np.uint32), rows[:, 3:].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [4, 5])
@pytest.mark.parametrize("name", CASES)
def test_keep_mask_equals_the_reference_flags(hip, golden, name, cols, tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_calib
    db, path, xyz, uv_ref = _case(golden, name, tmp_path)
    m = lidar_calib.load_projection(path, db)
    rows = _rows(xyz, cols, seed=cols)
    want = _flags(uv_ref, IMG_SIZE[db])
    unsure = _near_edge(uv_ref, IMG_SIZE[db], BAND[db])
    print("%s: %d points, %d inside, %d within the band of an edge" % (name, len(want), want.sum(), unsure.sum()))
    assert unsure.sum() <= 1e-4 * len(want)
    _, got, kept = _filter(rows, m, IMG_SIZE[db])
    alive = ~np.isnan(got[:, 0])
    np.testing.assert_array_equal(alive[~unsure], want[~unsure])
    _check_filtered(got, rows, alive)
    assert kept == int(alive.sum())                                                 # the range is wide open


@pytest.mark.gpu
def test_fov_semantics_on_small_integer_matrices(hip):
    """No depth test, the division, and the half-open frame: u = x / z, v = y / z on a 4 x 8 frame, then a matrix with a
    translation column.  Every value is exact in float32 and float64."""
    inf, nan = float("inf"), float("nan")
    m = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64)
    named = [
        ((2, 1, 1), True),            # plainly inside
        ((-4, -2, -2), True),         # BEHIND the camera (h2 < 0), quotient (2, 1) inside: kept, the reference has no depth test
        ((4, 2, -2), False),          # behind, quotient (-2, -1)
        ((1, 1, 0), False),           # h2 == 0: +inf
        ((-1, 1, 0), False),          # h2 == 0: -inf
        ((0, 0, 0), False),           # 0 / 0
        ((nan, 1, 1), False), ((1, nan, 1), False), ((1, 1, nan), False),
        ((inf, 1, 1), False), ((-inf, 1, 1), False), ((1, inf, 1), False), ((1, 1, inf), False), ((1, 1, -inf), False),
        ((0, 1, 1), True),            # u == 0 exactly
        ((1, 0, 1), True),            # v == 0 exactly
        ((-0.0, 1, 1), True),         # -0.0 >= 0
        ((8, 1, 1), False),           # u == img_w exactly
        ((1, 4, 1), False),           # v == img_h exactly
        ((16, 2, 2), False),          # u == img_w through the division
        ((np.float32(7.9999995), 1, 1), True), ((1, np.float32(3.9999998), 1), True),
        ((-1e-30, 1, 1), False), ((1, -1e-30, 1), False),
        ((3e38, 1e38, 1e38), True),   # large but finite: u = 3, v = 1
    ]
    rows = np.zeros((len(named), 4), np.float32)
    rows[:, :3] = np.array([p for p, _ in named], np.float32)
    rows[:, 3] = np.arange(len(named))
    want = np.array([k for _, k in named])
    uv, _ = _project(m, rows[:, :3])
    np.testing.assert_array_equal(_flags(uv, [4, 8]), want)                         # numpy float64 decides the same
    _, got, kept = _filter(rows, m, [4, 8])
    alive = ~np.isnan(got[:, 0])
    assert alive.tolist() == want.tolist(), [named[i] for i in np.where(alive != want)[0]]
    np.testing.assert_array_equal(got[alive].view(np.uint32), rows[alive].view(np.uint32))
    np.testing.assert_array_equal(got[:, 3], rows[:, 3])
    assert kept == int(want.sum())
    # a full matrix: h = [2x + y + 1, y + 3z - 2, x + 2]
    m2 = np.array([[2, 1, 0, 1], [0, 1, 3, -2], [1, 0, 0, 2]], np.float64)
    rng = np.random.default_rng(5)
    rows2 = np.zeros((4096, 4), np.float32)
    rows2[:, :3] = rng.integers(-8, 9, (4096, 3))
    rows2[:5, :3] = [[-2, 1, 1], [-2, 3, 0], [-1, 1, 1], [-3, 4, -1], [6, 3, 1]]   # h2 = 0 (2x), u = 0, behind & inside, u = 16/8
    uv2, h2 = _project(m2, rows2[:, :3])
    want2 = _flags(uv2, [5, 2])
    assert not want2[:2].any() and want2[2] and want2[3] and h2[3] < 0 and not want2[4]
    assert (want2 & (h2 < 0)).sum() > 50 and (h2 == 0).sum() > 50
    _, got2, kept2 = _filter(rows2, m2, [5, 2])
    np.testing.assert_array_equal(~np.isnan(got2[:, 0]), want2)
    assert kept2 == int(want2.sum())


def _scan(n, seed, cols=4):
    """A scan around the sensor: every octant, ~half of the forward points inside the KITTI frame."""
    rng = np.random.default_rng(seed)
    pts = np.stack((rng.uniform(-30, 75, n), rng.uniform(-45, 45, n), rng.uniform(-3.3, 3.3, n), rng.uniform(0, 3, n),
                    rng.uniform(0, 2, n)), 1).astype(np.float32)
    dense = n // 8
    pts[:dense, :3] = rng.normal([14, 1, -1], [0.08, 0.08, 0.3], (dense, 3))       # voxels with > 32 points, inside the frame
    return np.ascontiguousarray(pts[rng.permutation(n)][:, :cols])


def _kitti(golden, tmp_path, name="kitti_plain"):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_calib
    db, path, _, _ = _case(golden, name, tmp_path)
    return lidar_calib.load_projection(path, db), IMG_SIZE[db]


STEPS = {
    "none": LidarAugment(seed=3),
    "flip_x": LidarAugment(flip_x=True), "flip_y": LidarAugment(flip_y=True), "swap": LidarAugment(swap_xy=True),
    "rotate": LidarAugment(rotation=0.35), "gauss": LidarAugment(gauss=(0.06, 0.04, 0.03), seed=21),
    "dropout": LidarAugment(p_keep=0.85, seed=22), "rain": LidarAugment(rain_rate=10.0, rain_max_range=120.0, seed=23),
    "test_dropout": LidarAugment(test_dropout=True, seed=24),
    "all": LidarAugment(flip_x=True, flip_y=True, swap_xy=True, rotation=0.4, gauss=(0.06, 0.06, 0.04), p_keep=0.85,
                        rain_rate=10.0, rain_max_range=120.0, test_dropout=True, seed=25),
}


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [4, 5])
@pytest.mark.parametrize("step", sorted(STEPS))
def test_fused_pass_equals_filter_then_old_entry(hip, golden, tmp_path, step, cols):
    """frcnn_lidar_augment_fov(record) == field of view alone, then the OLD frcnn_lidar_augment(record, same seed), bit for
    bit, kept_count included: both index their draws by the row in the file."""
    m, size = _kitti(golden, tmp_path)
    aug = STEPS[step]
    rows = _scan(30000, seed=len(step) + cols, cols=cols)
    dev = torch.from_numpy(rows).to(DEV)
    fused, kept = ops.lidar_augment_points(dev, aug, aug.seed, EXTENTS, proj=m, img_size=size)
    only, n_fov = ops.lidar_fov_filter(dev, m, size)
    two, kept2 = ops.lidar_augment_points(only, aug, aug.seed, EXTENTS)              # the old entry
    torch.cuda.synchronize()
    a, b = fused.cpu().numpy(), two.cpu().numpy()
    assert a.tobytes() == b.tobytes() and int(kept.item()) == int(kept2.item())
    alive = ~np.isnan(a[:, 0])
    in_fov = ~np.isnan(only.cpu().numpy()[:, 0])
    uv, _ = _project(m, rows[:, :3])
    np.testing.assert_array_equal(in_fov, _flags(uv, size))                         # (no point of this cloud is near an edge)
    assert not _near_edge(uv, size, BAND["kitti"]).any() and int(n_fov.item()) == int(in_fov.sum())
    assert 0 < alive.sum() < in_fov.sum() < len(rows) and not alive[~in_fov].any()
    assert 0 < int(kept.item()) <= alive.sum()
    np.testing.assert_array_equal(a[:, 4:], rows[:, 4:])
    if step in ("dropout", "test_dropout"):
        # the draw of a surviving candidate is the draw of its FILE row, whatever the filter removed before it
        x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
        cand = in_fov & (x >= 0) & (y >= -40) & (z >= -3) & (x < 70) & (y < 40) & (z < 3)
        p = np.float32(0.85 if step == "dropout" else 0.8)
        draws = O.uniform01(aug.seed, ops.AUG_STREAM[step], np.arange(len(rows)))
        np.testing.assert_array_equal(alive, cand & (draws < p))
        compacted = O.uniform01(aug.seed, ops.AUG_STREAM[step], np.maximum(np.cumsum(in_fov) - 1, 0))
        assert not np.array_equal(alive, cand & (compacted < p))
    # the grid shape does not matter, in place works
    for blocks in (1, 7):
        c, kc = ops.lidar_augment_points(dev, aug, aug.seed, EXTENTS, proj=m, img_size=size, max_blocks=blocks)
        assert c.cpu().numpy().tobytes() == a.tobytes() and int(kc.item()) == int(kept.item())
    same, ks = ops.lidar_augment_points(dev, aug, aug.seed, EXTENTS, out=dev, proj=m, img_size=size)
    assert same is dev and dev.cpu().numpy().tobytes() == a.tobytes() and int(ks.item()) == int(kept.item())


@pytest.mark.gpu
def test_old_entry_is_unchanged(hip):
    """``ops.lidar_augment_points`` without ``proj`` still calls frcnn_lidar_augment: equal to the direct C call, and to the
    float32 restatement of a flip (x' = -x + 70 on the rows inside the range, NaN elsewhere)."""
    lib = hip
    rows = _scan(30000, seed=9)
    aug = LidarAugment(flip_x=True, p_keep=0.9, seed=77)
    dev = torch.from_numpy(rows).to(DEV)
    got, kept = ops.lidar_augment_points(dev, aug, aug.seed, EXTENTS)
    out, cnt = torch.empty_like(dev), torch.empty((1,), dtype=torch.int32, device=DEV)
    vals = _hip.float_array([0, 0, 0, 0.9, 1, 0, 0, 0])
    rc = lib.frcnn_lidar_augment(dev.data_ptr(), 30000, 4, _hip.float_array(EXTENTS), ops.AUG_DROPOUT | ops.AUG_FLIP_X, vals,
                                 77, None, out.data_ptr(), cnt.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == out.cpu().numpy().tobytes() and int(kept.item()) == int(cnt.item())
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    keep = (x >= 0) & (y >= -40) & (z >= -3) & (x < 70) & (y < 40) & (z < 3)
    keep &= O.uniform01(77, ops.AUG_STREAM["dropout"], np.arange(30000)) < np.float32(0.9)
    want = rows.copy()
    want[:, 0] = -x + np.float32(70)
    g = got.cpu().numpy()
    np.testing.assert_array_equal(~np.isnan(g[:, 0]), keep)
    np.testing.assert_array_equal(g[keep].view(np.uint32), want[keep].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [4, 5])
def test_bev_of_nan_rows_equals_bev_of_the_compacted_cloud(hip, golden, tmp_path, cols):
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.minibatch import get_lidar_blob
    m, size = _kitti(golden, tmp_path, "kitti_tilted")
    rows = _scan(30000, seed=13, cols=cols)
    uv, _ = _project(m, rows[:, :3])
    flag = _flags(uv, size)
    dev, got, _ = _filter(rows, m, size)
    np.testing.assert_array_equal(~np.isnan(got[:, 0]), flag)
    elong = 4 if cols == 5 else None
    for max_voxels in (25000, 2000):                                # the cap makes voxel numbering (row order) matter
        C.cfg.LIDAR.MAX_NUM_VOXEL = max_voxels
        _, a = get_lidar_blob(dev, 0.5, device=DEV, elongation=elong)
        _, b = get_lidar_blob(np.ascontiguousarray(rows[flag]), 0.5, device=DEV, elongation=elong)
        _, raw = get_lidar_blob(rows, 0.5, device=DEV, elongation=elong)
        assert torch.equal(a, b) and not torch.equal(a, raw)
        assert int((a[..., :12] != 0).sum()) > 500


def _write_frame(root, db, name, rows, calib_text):
    scan_dir = root / ("velodyne" if db == "kitti" else "point_clouds")
    os.makedirs(str(scan_dir), exist_ok=True)
    os.makedirs(str(root / "calib"), exist_ok=True)
    path = str(scan_dir / (name + ".bin"))
    rows.astype(np.float32).tofile(path)
    with open(str(root / "calib" / (name + ".txt")), "w") as f:
        f.write(calib_text)
    return path


def _seed_with(pred):
    for s in range(2000):
        if pred(draw_lidar_augmentation(np.random.default_rng(s))):
            return s
    raise AssertionError("no generator seed found")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kitti_plain", "cadc_plain"])
def test_data_layer_end_to_end(hip, golden, tmp_path, name):
    import test_lidar_augment as TA
    from faster_rcnn_pytorch_multimodal_amd.model.test import _get_blobs
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_calib, minibatch
    from faster_rcnn_pytorch_multimodal_amd.utils.bbox import bbox_pc_to_voxel_grid
    db = str(golden[name + "_db"])
    text = str(golden[name + "_calib"])
    C.cfg.DB_NAME = db
    C.cfg.TRAIN.SCALES = (0.5,)
    C.cfg.TEST.SCALES = (0.5,)
    rows = _scan(30000, seed=31)
    path = _write_frame(tmp_path, db, "000007", rows, text)
    m = lidar_calib.load_projection(lidar_calib.calib_filename(path, db), db)
    size = IMG_SIZE[db]
    uv, _ = _project(m, rows[:, :3])
    flag = _flags(uv, size)
    assert not _near_edge(uv, size, BAND[db]).any() and 3000 < flag.sum() < 27000
    _, want = minibatch.get_lidar_blob(np.ascontiguousarray(rows[flag]), 0.5, device=DEV)      # the reference's points[fov_flag]
    _, raw = minibatch.get_lidar_blob(rows, 0.5, device=DEV)
    assert not torch.equal(want, raw)
    # test mode and train / val mode without augmentation: the filter alone
    infos, blob, local = minibatch._get_lidar_blob([path], EXTENTS, 0.5, augment_en=False, mode='test')
    assert local is None and torch.equal(blob, want) and infos[0].tolist() == [0, 350, 0, 400, 0, 12, 0.5]
    entry = TA._entry(path)
    for mode in ('train', 'val'):
        _, blob, local = minibatch._get_lidar_blob([entry], EXTENTS, 0.5, augment_en=False, mode=mode)
        assert torch.equal(blob, want)
        np.testing.assert_array_equal(local[0]['boxes'], entry['boxes'])            # the gt boxes are not touched
    assert torch.equal(_get_blobs([path])['data'], want)                             # what test_net calls per frame
    # the same scan under another DB_NAME: no filter (the Waymo path)
    C.cfg.DB_NAME = 'waymo'
    assert torch.equal(minibatch._get_lidar_blob([path], EXTENTS, 0.5, augment_en=False, mode='test')[1], raw)
    C.cfg.DB_NAME = db
    # test mode honours the rain simulation and the test dropout, in the same pass
    C.cfg.TEST.RAIN_SIM_EN, C.cfg.TEST.RAIN_RATE, C.cfg.TEST.DROPOUT_EN = True, 10, True
    LA.set_augmentation_rng(np.random.default_rng(1))
    aug = draw_lidar_augmentation(np.random.default_rng(1), augment_en=False, mode='test')
    assert aug.rain_rate == 10.0 and aug.test_dropout and aug.rain_max_range == float(C.cfg[db.upper()].LIDAR_MAX_RANGE)
    _, rained, _ = minibatch._get_lidar_blob([path], EXTENTS, 0.5, augment_en=False, mode='test')
    moved, _ = ops.lidar_augment_points(torch.from_numpy(rows).to(DEV), aug, aug.seed, EXTENTS, proj=m, img_size=size)
    assert torch.equal(rained, minibatch.get_lidar_blob(moved, 0.5, device=DEV)[1]) and not torch.equal(rained, want)
    C.cfg.TEST.RAIN_SIM_EN, C.cfg.TEST.DROPOUT_EN = False, False
    # get_minibatch without and with the training augmentation
    plain = minibatch.get_minibatch([entry], 2, False, 0)
    assert torch.equal(plain['data'], want) and plain['flipped'] is False and plain['filename'] == path
    seed = _seed_with(lambda a: a.flip_x and a.gauss is not None and a.p_keep is not None)
    aug = draw_lidar_augmentation(np.random.default_rng(seed))
    LA.set_augmentation_rng(np.random.default_rng(seed))
    before = copy.deepcopy(entry)
    blobs = minibatch.get_minibatch([entry], 2, True, 0)
    np.testing.assert_array_equal(entry['boxes'], before['boxes'])
    moved, _ = ops.lidar_augment_points(torch.from_numpy(rows).to(DEV), aug, aug.seed, EXTENTS, proj=m, img_size=size)
    assert torch.equal(blobs['data'], minibatch.get_lidar_blob(moved, 0.5, device=DEV)[1])
    assert not torch.equal(blobs['data'], want) and blobs['flipped'] is True
    moved_entry = augment_gt_boxes(copy.deepcopy(entry), aug)
    inds = np.where(np.asarray(moved_entry['ignore']) == 0)[0]
    gt = np.empty((len(inds), 8), np.float32)
    gt[:, :7] = bbox_pc_to_voxel_grid(np.array(moved_entry['boxes'], dtype=np.float64)[inds], EXTENTS, blobs['info'])
    gt[:, 0:2] *= 0.5
    gt[:, 3:5] *= 0.5
    gt[:, 7] = moved_entry['gt_classes'][inds]
    np.testing.assert_array_equal(blobs['gt_boxes'], gt)
    # the roidb entry's 'calib' key wins over the derived name
    other = "kitti_tilted" if db == "kitti" else "cadc_skewed"
    _, other_path, _, _ = _case(golden, other, tmp_path)
    m2 = lidar_calib.load_projection(other_path, db)
    flag2 = _flags(_project(m2, rows[:, :3])[0], size)
    keyed = dict(entry, calib=other_path)
    _, blob2, _ = minibatch._get_lidar_blob([keyed], EXTENTS, 0.5, augment_en=False)
    assert torch.equal(blob2, minibatch.get_lidar_blob(np.ascontiguousarray(rows[flag2]), 0.5, device=DEV)[1])
    assert not torch.equal(blob2, want)
    # a frame whose points all fall outside the image is skipped like the reference's "no points left"
    outside = rows[~flag][:5000]
    empty = _write_frame(tmp_path, db, "000008", outside, text)
    infos, blob, local = minibatch._get_lidar_blob([empty], EXTENTS, 0.5, augment_en=False, mode='test')
    assert infos == [] and blob is None and local is None
    infos, blob, local = minibatch._get_lidar_blob([TA._entry(empty)], EXTENTS, 0.5, augment_en=False)
    assert infos == [] and blob is None and local[0]['filename'] == empty
    assert minibatch.get_minibatch([TA._entry(empty)], 2, False, 0) is None
    LA.set_augmentation_rng(np.random.default_rng(seed))
    assert minibatch.get_minibatch([TA._entry(empty)], 2, True, 0) is None
    # a missing calibration file is an error, not a silent pass-through
    orphan = str(tmp_path / "orphan.bin")
    rows.tofile(orphan)
    with pytest.raises(OSError):
        minibatch._get_lidar_blob([orphan], EXTENTS, 0.5, augment_en=False, mode='test')


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kitti_plain", "cadc_plain"])
def test_lidar_train_step_on_a_filtered_scan(hip, golden, tmp_path, name):
    """``train_net`` on ``.bin`` scans of a camera dataset: the data layer filters, augments and the detector trains."""
    import test_lidar_augment as TA
    from faster_rcnn_pytorch_multimodal_amd.model.config import get_output_dir, get_output_tb_dir
    from faster_rcnn_pytorch_multimodal_amd.model.train_val import train_net
    from faster_rcnn_pytorch_multimodal_amd.nets.lidarnet import lidarnet
    from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
    cfg = C.cfg
    db_name = str(golden[name + "_db"])
    cfg.DB_NAME = db_name
    cfg.ROOT_DIR = str(tmp_path)
    cfg.TRAIN.SCALES = (0.5,)
    cfg.TRAIN.SNAPSHOT_ITERS = 1000
    cfg.TRAIN.LEARNING_RATE = 1e-5
    cfg.TRAIN.GRAPHS = False              # eager steps: what is under test here is the data layer feeding the step
    roidb = [TA._entry(_write_frame(tmp_path, db_name, "%06d" % i, _scan(20000, seed=40 + i), str(golden[name + "_calib"])))
             for i in range(2)]

    class Db:
        name = "synthetic_lidar_fov_train"
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


@pytest.mark.gpu
def test_capture_replay_and_launch_count(hip, golden, tmp_path):
    """The new entry captured in a hipGraph and replayed equals the eager call (the seed word and the points may change
    between replays); the capture holds kernel nodes only, and no more of them than the augment-only call."""
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import capture
    from faster_rcnn_pytorch_multimodal_amd.model.train_graph import graph_node_kinds
    m, size = _kitti(golden, tmp_path)
    aug = STEPS["all"]
    rows = _scan(30000, seed=51)
    static_in = torch.from_numpy(rows).to(DEV)
    static_out = torch.empty_like(static_in)
    word = torch.zeros((1,), dtype=torch.int32, device=DEV)
    eager, eager_kept = ops.lidar_augment_points(static_in, aug, aug.seed, EXTENTS, seed_dev=word, proj=m, img_size=size)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    counts = {}
    graphs = {}
    kept = {}
    for kind in ("fov", "old"):
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with capture(g, stream=stream):
            if kind == "fov":
                _, kept[kind] = ops.lidar_augment_points(static_in, aug, aug.seed, EXTENTS, seed_dev=word, out=static_out,
                                                         proj=m, img_size=size)
            else:
                _, kept[kind] = ops.lidar_augment_points(static_in, aug, aug.seed, EXTENTS, seed_dev=word,
                                                         out=torch.empty_like(static_in))
        hist, nodes, edges = graph_node_kinds(g)
        print("%s: %s" % (kind, hist))
        assert set(hist) == {"kernel"} and edges == nodes - 1, hist
        counts[kind] = nodes
        g.instantiate()
        graphs[kind] = g
    assert counts["fov"] <= counts["old"] and counts["fov"] <= 2, counts           # the pass, plus the counter clear
    with torch.cuda.stream(stream):
        graphs["fov"].replay()
    torch.cuda.synchronize()
    assert _same_bytes(static_out, eager) and int(kept["fov"].item()) == int(eager_kept.item())
    # new points and a new seed word: the replay follows
    rows2 = _scan(30000, seed=52)
    static_in.copy_(torch.from_numpy(rows2))
    word.fill_(5)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        graphs["fov"].replay()
    torch.cuda.synchronize()
    eager2, eager2_kept = ops.lidar_augment_points(torch.from_numpy(rows2).to(DEV), aug, aug.seed + 5, EXTENTS, proj=m,
                                                   img_size=size)
    torch.cuda.synchronize()
    assert _same_bytes(static_out, eager2) and int(kept["fov"].item()) == int(eager2_kept.item())
    assert not _same_bytes(eager2, eager)
