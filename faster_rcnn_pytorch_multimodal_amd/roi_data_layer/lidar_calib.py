"""Camera calibration of a KITTI / CADC LiDAR frame for the field-of-view filter (lib/roi_data_layer/minibatch.py:251-268,
678-693): a calibration file becomes ONE float64 3x4 matrix ``M`` that takes a homogeneous LiDAR point ``[x, y, z, 1]``
to the homogeneous pixel ``[h0, h1, h2]`` of the front camera, ``u = h0 / h2``, ``v = h1 / h2``.  The per-point side
(projection, the four comparisons of ``get_fov_flag``) runs on the device as the first step of
``frcnn_lidar_augment_fov`` (``ops.lidar_augment_points(..., proj=M, img_size=...)``, ``ops.lidar_fov_filter``).

KITTI (lib/utils/kitti_utils.py:108-149,177-215): ``M = P2 . [R0_rect 0; 0 1] . [Tr_velo_to_cam; 0 0 0 1]``; the
reference chains the three products over the whole cloud, which differs from the composite by rounding only.
CADC (lib/utils/CADC_utils.py:13-48): ``M`` = the first three rows of ``K4 . inv(T_LIDAR_CAM00)``, both matrices parsed as
float32 like the reference does, ``K4`` = ``CAM00_matrix`` inside an identity 4x4.  Only the front camera (``P2`` /
``CAM00``) is read.
"""
import numpy as np

from ..model.config import cfg

FOV_DATASETS = ('kitti', 'cadc')


def calib_filename(scan_filename, db_name):
    """The reference's derivation of the calibration file from the scan's path (minibatch.py:254,260)."""
    name = str(scan_filename)
    if db_name == 'kitti':
        return name.replace('velodyne', 'calib').replace('.bin', '.txt')
    if db_name == 'cadc':
        return name.replace('point_clouds', 'calib').replace('.bin', '.txt')
    raise ValueError("no camera calibration convention for cfg.DB_NAME %r (expected one of %s)" % (db_name, FOV_DATASETS))


def _matrix(values, shape, filename, key):
    if len(values) != shape[0] * shape[1]:
        raise ValueError("%s: %s holds %d values, a %dx%d matrix needs %d"
                         % (filename, key, len(values), shape[0], shape[1], shape[0] * shape[1]))
    m = np.asarray(values).reshape(shape)
    if not np.isfinite(m).all():
        raise ValueError("%s: %s holds a value that is not finite" % (filename, key))
    return m


def read_kitti_calib_file(filename):
    """``{key: float64 array}`` of the ``key: floats`` lines; lines whose values are not floats (dates) are skipped
    (kitti_utils.py:132-149)."""
    data = {}
    with open(filename, 'r') as f:
        for line in f.readlines():
            line = line.rstrip()
            if len(line) == 0 or ':' not in line:
                continue
            key, value = line.split(':', 1)
            try:
                data[key] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass
    return data


def kitti_projection(filename):
    """3x4 float64 ``M = P2 . [R0_rect 0; 0 1] . [Tr_velo_to_cam; 0 0 0 1]`` of a KITTI object calibration file."""
    data = read_kitti_calib_file(filename)
    for key in ('P2', 'R0_rect', 'Tr_velo_to_cam'):
        if key not in data:
            raise ValueError("%s: calibration key %s is missing" % (filename, key))
    p2 = _matrix(data['P2'], (3, 4), filename, 'P2')
    r0, tr = np.eye(4), np.eye(4)
    r0[:3, :3] = _matrix(data['R0_rect'], (3, 3), filename, 'R0_rect')
    tr[:3, :] = _matrix(data['Tr_velo_to_cam'], (3, 4), filename, 'Tr_velo_to_cam')
    return np.ascontiguousarray(p2 @ r0 @ tr)


def cadc_projection(filename):
    """3x4 float64 ``M`` = the first three rows of ``K4 . inv(T_LIDAR_CAM00)`` of a CADC per-frame calibration file (the
    tokens after ``T_LIDAR_CAM00:`` and ``CAM00_matrix:``, read as float32 like CADC_utils.py:34,36)."""
    found = {}
    with open(filename, 'r') as f:
        for line in f.read().splitlines():
            tokens = line.rstrip().split(' ')
            if tokens[0] in ('T_LIDAR_CAM00:', 'CAM00_matrix:'):
                key = tokens[0][:-1]
                try:
                    found[key] = np.array([t for t in tokens[1:] if t != '']).astype(np.float32)
                except ValueError:
                    raise ValueError("%s: %s holds a token that is not a number" % (filename, key))
    for key in ('T_LIDAR_CAM00', 'CAM00_matrix'):
        if key not in found:
            raise ValueError("%s: calibration key %s is missing" % (filename, key))
    extrinsic = _matrix(found['T_LIDAR_CAM00'], (4, 4), filename, 'T_LIDAR_CAM00')
    k4 = np.eye(4)
    k4[0:3, 0:3] = _matrix(found['CAM00_matrix'], (3, 3), filename, 'CAM00_matrix')
    try:
        inverse = np.linalg.inv(extrinsic)          # of the float32 matrix, like the reference (CADC_utils.py:24)
    except np.linalg.LinAlgError:
        raise ValueError("%s: T_LIDAR_CAM00 is singular" % filename)
    return np.ascontiguousarray(np.matmul(k4, inverse)[0:3, :], dtype=np.float64)


def load_projection(calib_file, db_name):
    """``M`` of ``calib_file`` in the format of ``db_name`` ('kitti' or 'cadc')."""
    if db_name == 'kitti':
        return kitti_projection(calib_file)
    if db_name == 'cadc':
        return cadc_projection(calib_file)
    raise ValueError("no camera calibration convention for cfg.DB_NAME %r (expected one of %s)" % (db_name, FOV_DATASETS))


def frame_projection(scan_filename, entry=None, db_name=None):
    """(M, [height, width]) of one frame: the calibration file is ``entry['calib']`` when the roidb entry carries that
    optional key, else derived from the scan's path like the reference; the frame size is cfg.<DB_NAME>.IMG_SIZE."""
    db_name = cfg.DB_NAME if db_name is None else db_name
    calib_file = entry['calib'] if isinstance(entry, dict) and entry.get('calib') else calib_filename(scan_filename, db_name)
    img_size = [int(v) for v in cfg[str(db_name).upper()].IMG_SIZE]
    return load_projection(calib_file, db_name), img_size


def project_points(proj, xyz):
    """Host restatement of the device step (float64): pixel coordinates (N, 2) of ``xyz`` (N, 3) under ``proj``.  For
    checks and tools; the data layer does not call it."""
    xyz = np.asarray(xyz, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        h = np.concatenate((xyz, np.ones((xyz.shape[0], 1))), 1) @ np.asarray(proj, dtype=np.float64).T
        return h[:, 0:2] / h[:, 2:3]


def fov_flags(pixels, img_size):
    """``get_fov_flag`` (minibatch.py:689-691) on pixel coordinates: ``img_size`` = [height, width]."""
    return (pixels[:, 0] >= 0) & (pixels[:, 0] < img_size[1]) & (pixels[:, 1] >= 0) & (pixels[:, 1] < img_size[0])
