"""LiDAR input producer - counterpart of ``_get_lidar_blob`` (lib/roi_data_layer/minibatch.py:237-516) for ONE frame
whose points are already in memory: range filter (:232-235), voxelisation and the BEV scatter (:434-512) run as
``frcnn_bev_voxelize`` on the device, the per-point augmentations and the test-time rain simulation in front of them
(:274-428) as ``frcnn_lidar_augment``; the caller parses the file and, for a KITTI / CADC scan, applies the camera
field-of-view filter (:250-273; ``_get_lidar_blob`` below does both).  Returns the same ``(infos, blob)`` the reference's data layer hands to
``Network.forward``: blob (1, num_y_voxel, num_x_voxel, cfg.LIDAR.NUM_CHANNEL) NHWC on the device,
info = [0, num_x_voxel, 0, num_y_voxel, 0, NUM_SLICES, scale].

The reference-named entry points (``_get_image_blob``, ``_get_lidar_blob``, ``get_minibatch``: what
``lib/model/test.py:32-44`` and ``lib/roi_data_layer/layer.py:66-82`` call) load ONE frame from a file and hand it to the
device producers (``frcnn_prep_image``, ``frcnn_lidar_augment``, ``frcnn_bev_voxelize``).  LiDAR frames: ``augment_en=True``
draws the reference's flips / distortion / dropout / rotation / swap per frame (``roi_data_layer/lidar_augment.py``),
moves the points on the device and the gt boxes on the host; ``mode='test'`` applies cfg.TEST.RAIN_SIM_EN / DROPOUT_EN.
KITTI / CADC ``.bin`` scans (``cfg.DB_NAME``) are first cut to the front camera's field of view (:251-268,678-693): the
calibration file is read on the host (``roi_data_layer/lidar_calib.py``), the projection and the test run on the device
as the first step of the same per-point pass (``frcnn_lidar_augment_fov``).
Image frames: with ``cfg.IMAGE.EN_AUG`` on, ``augment_en=True`` draws the reference's flip / blur-sharpen / noise /
hue-saturation / affine / dropout per frame (``roi_data_layer/image_augment.py``, minibatch.py:540-647), runs the pixels
through ``frcnn_image_augment`` on the device in front of ``frcnn_prep_image`` and moves, clips and flags the gt boxes on
the host.  The switch defaults to off: ``augment_en=True`` then raises for images.  The test-time ``Spatter`` corruption
(:648-664, ``augment_en=True`` with ``mode='test'``: what cfg.TEST.AUGMENT_EN asks for) is behind ``cfg.IMAGE.EN_TEST_SPATTER``
in the same way: on, the frame goes through ``frcnn_image_spatter`` on the device in front of ``frcnn_prep_image``; off, it raises.
"""
import numpy as np
import torch

from .. import ops
from ..model.config import cfg


def lidar_frame_geometry(scale):
    """Voxel size, shifted point-cloud range and info vector of a frame (minibatch.py:434-451)."""
    voxel_len = cfg.LIDAR.VOXEL_LEN / scale
    num_x_voxel = int((cfg.LIDAR.X_RANGE[1] - cfg.LIDAR.X_RANGE[0]) * (1 / voxel_len))
    num_y_voxel = int((cfg.LIDAR.Y_RANGE[1] - cfg.LIDAR.Y_RANGE[0]) * (1 / voxel_len))
    vertical = (cfg.LIDAR.Z_RANGE[1] - cfg.LIDAR.Z_RANGE[0]) / (cfg.LIDAR.NUM_SLICES + 0.0)
    assert vertical == cfg.LIDAR.VOXEL_HEIGHT
    # pc_extents shifted so that the grid starts at z = 0 (:441-443)
    pc_range = [cfg.LIDAR.X_RANGE[0], cfg.LIDAR.Y_RANGE[0], 0.0, cfg.LIDAR.X_RANGE[1], cfg.LIDAR.Y_RANGE[1],
                cfg.LIDAR.Z_RANGE[1] - cfg.LIDAR.Z_RANGE[0]]
    info = np.array([0, num_x_voxel, 0, num_y_voxel, 0, int(cfg.LIDAR.NUM_SLICES), scale], dtype=np.float32)
    return [voxel_len, voxel_len, cfg.LIDAR.VOXEL_HEIGHT], pc_range, info


def get_lidar_blob(points, scale, device='cuda', elongation=None):
    """points: (N, >=4) float32 rows [x, y, z, intensity, (elongation)] in file order (numpy or device tensor).
    ``elongation``: column index of the elongation value (Waymo, minibatch.py:496-499) or None (channel = tanh(0))."""
    if isinstance(points, np.ndarray):
        points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(device, non_blocking=True)
    voxel_size, pc_range, info = lidar_frame_geometry(scale)
    num_meta = int(cfg.LIDAR.NUM_META_CHANNEL)
    if int(cfg.LIDAR.NUM_SLICES) + num_meta != int(cfg.LIDAR.NUM_CHANNEL):
        raise ValueError("cfg.LIDAR.NUM_CHANNEL must equal NUM_SLICES + NUM_META_CHANNEL")
    bev, _ = ops.bev_voxelize(points.contiguous(), pc_range, voxel_size, cfg.LIDAR.Z_RANGE[0],
                              cfg.LIDAR.MAX_PTS_PER_VOXEL, cfg.LIDAR.MAX_NUM_VOXEL, cfg.LIDAR.NUM_SLICES, num_meta,
                              -1 if elongation is None else int(elongation))
    if (bev.shape[0], bev.shape[1]) != (int(info[3]), int(info[1])):
        raise RuntimeError("voxel grid %s does not match the info vector %s" % (tuple(bev.shape), info.tolist()))
    return [info.tolist()], bev.unsqueeze(0)


# ---------------------------------------------------------------------------------------------------------------
# reference-named loaders
# ---------------------------------------------------------------------------------------------------------------
def read_image_file(filename):
    """uint8 (H, W, 3) array in BGR channel order - what ``cv2.imread`` returns (minibatch.py:529,532).  ``.npy`` files
    hold that array directly; anything else is decoded with PIL (cv2 is not a dependency of this package)."""
    if str(filename).endswith('.npy'):
        im = np.load(filename)
    else:
        from PIL import Image
        with Image.open(filename) as f:
            im = np.asarray(f.convert('RGB'))[:, :, ::-1]
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
        raise ValueError("%s: expected a uint8 (H, W, 3) image, got %s %s" % (filename, im.dtype, im.shape))
    return np.ascontiguousarray(im)


def read_point_cloud_file(filename):
    """(N, >=4) float32 rows [x, y, z, intensity, ...]: ``.bin`` = flat float32 quadruples, ``.npy`` as stored
    (minibatch.py:251-270).  The raw rows of the file whatever the dataset: the camera field-of-view filter of KITTI /
    CADC scans (:253-264) runs on the device afterwards (``_get_lidar_blob``)."""
    if '.bin' in str(filename):
        return np.fromfile(filename, dtype=np.float32).reshape(-1, 4)
    if '.npy' in str(filename):
        return np.load(filename)
    raise ValueError('Cannot handle this type of binary file: %s' % filename)


def _no_augmentation(augment_en, mode='train'):
    if augment_en and mode == 'test':
        if not cfg.IMAGE.EN_TEST_SPATTER:
            raise NotImplementedError("augment_en=True with mode='test': the imgcorruptlike Spatter corruption of "
                                      "lib/roi_data_layer/minibatch.py:648-664 is behind cfg.IMAGE.EN_TEST_SPATTER, which "
                                      "is False; set it or pass augment_en=False")
        return
    if augment_en and not cfg.IMAGE.EN_AUG:
        raise NotImplementedError("augment_en=True: image augmentation (lib/roi_data_layer/minibatch.py:540-647, "
                                  "roi_data_layer/image_augment.py) is behind cfg.IMAGE.EN_AUG, which is False; set it "
                                  "or pass augment_en=False")


def _get_image_blob(roidb, im_scale, augment_en=False, mode='train', device='cuda'):
    """minibatch.py:518-676.  ``roidb``: list with ONE filename (mode 'test') or ONE roidb entry (dict with 'filename').
    Returns (im_infos, blob (1, H', W', 3) float32 device tensor, local_roidb).  ``augment_en`` (train / val mode, behind
    cfg.IMAGE.EN_AUG): file -> uint8 frame on the device -> ``frcnn_image_augment`` (skipped for an identity draw) ->
    ``frcnn_prep_image``; boxes, ``ignore`` and ``flipped`` of the local entry follow on the host.  ``augment_en`` in test
    mode (behind cfg.IMAGE.EN_TEST_SPATTER): file -> uint8 frame on the device -> ``frcnn_image_spatter`` ->
    ``frcnn_prep_image``, the seed of the draws from the frame's file name and cfg.RNG_SEED (``draw_test_corruption``)."""
    from copy import deepcopy
    from ..utils.blob import im_list_to_blob, prep_im_for_blob
    _no_augmentation(augment_en, mode)
    if len(roidb) != 1:
        raise NotImplementedError("single-frame batches only (minibatch.py:111)")
    if mode == 'test':
        im, local_roidb = read_image_file(roidb[0]), None
    else:
        im, local_roidb = read_image_file(roidb[0]['filename']), deepcopy(roidb)
        local_roidb[0]['flipped'] = False
    if augment_en and mode == 'test':
        from .image_augment import draw_test_corruption
        im = ops.image_spatter(torch.from_numpy(im).to(device, non_blocking=True), draw_test_corruption(key=roidb[0]))
    elif augment_en:
        from .image_augment import augment_image_gt_boxes, draw_image_augmentation
        height, width = int(im.shape[0]), int(im.shape[1])
        aug = draw_image_augmentation(width, height)
        if not aug.identity:
            im = ops.image_augment(torch.from_numpy(im).to(device, non_blocking=True), aug)
        augment_image_gt_boxes(local_roidb[0], aug, width, height)
    im = prep_im_for_blob(im, cfg.PIXEL_MEANS, cfg.PIXEL_STDDEVS, cfg.PIXEL_ARRANGE, im_scale, device=device)
    info = np.array([0, im.shape[1], 0, im.shape[0], 0, 0, im_scale], dtype=np.float32)          # :670
    return [info], im_list_to_blob([im]), local_roidb


def _get_lidar_blob(roidb, pc_extents, scale, augment_en=False, mode='train', device='cuda'):
    """minibatch.py:237-516: file -> points -> augmentation / rain simulation (``frcnn_lidar_augment``, only when a step
    is switched on) -> ``get_lidar_blob`` (range filter, voxel generator and BEV scatter on the device).  ``pc_extents`` is
    what the reference passes (cfg.LIDAR.*_RANGE); the voxeliser reads the same ranges from cfg.  Waymo scans carry the
    elongation in column 4 (:496-499).  A ``.bin`` scan with cfg.DB_NAME 'kitti' or 'cadc' goes through the camera
    field-of-view filter first (:253-264), in the same launch as the augmentation (``frcnn_lidar_augment_fov``; with no
    step switched on, that launch is the filter alone); its calibration file is derived from the scan's path like the
    reference does, or named by the roidb entry's optional 'calib' key.  The gt boxes are not touched by the filter.
    Returns (infos, None, local_roidb) when no point is left (:428-432)."""
    from copy import deepcopy
    from .lidar_calib import FOV_DATASETS, frame_projection
    from .lidar_augment import augment_gt_boxes, draw_lidar_augmentation
    if len(roidb) != 1:
        raise NotImplementedError("single-frame batches only (minibatch.py:111)")
    if cfg.LIDAR.SHUFFLE_PC:
        raise NotImplementedError("cfg.LIDAR.SHUFFLE_PC: the reference's line (minibatch.py:292-293) replaces the cloud by "
                                  "None and cannot run; keep it False")
    if mode == 'test':
        if augment_en:
            raise NotImplementedError("augment_en=True with mode='test': the reference flags a roidb entry there "
                                      "(minibatch.py:295) and a test frame has none; pass augment_en=False")
        filen, local_roidb = roidb[0], None
    else:
        filen, local_roidb = roidb[0]['filename'], deepcopy(roidb)
        local_roidb[0]['flipped'] = False
    expected = [cfg.LIDAR.X_RANGE[0], cfg.LIDAR.Y_RANGE[0], cfg.LIDAR.Z_RANGE[0],
                cfg.LIDAR.X_RANGE[1], cfg.LIDAR.Y_RANGE[1], cfg.LIDAR.Z_RANGE[1]]
    if [float(v) for v in pc_extents] != [float(v) for v in expected]:
        raise ValueError("pc_extents %s differ from cfg.LIDAR.*_RANGE %s" % (list(pc_extents), expected))
    points = read_point_cloud_file(filen)
    elongation = 4 if (cfg.DB_NAME == 'waymo' and points.shape[1] > 4) else None
    if cfg.DB_NAME in FOV_DATASETS and '.bin' in str(filen):
        proj, img_size = frame_projection(filen, None if local_roidb is None else local_roidb[0])
        aug = draw_lidar_augmentation(augment_en=augment_en, mode=mode)             # the identity record: the filter alone
        if points.shape[0] == 0:
            return [], None, local_roidb
        points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(device, non_blocking=True)
        points, kept = ops.lidar_augment_points(points, aug, aug.seed, expected, out=points, proj=proj, img_size=img_size)
        if local_roidb is not None and not aug.identity:
            augment_gt_boxes(local_roidb[0], aug)
        if int(kept.item()) <= 0:                                                    # :428-432
            print('No PC points in frame {} FLIP_X: {} FLIP_Y: {} ROT: {} SWAP_X_Y: {}'.format(
                filen, aug.flip_x, aug.flip_y, aug.rotation is not None, aug.swap_xy))
            return [], None, local_roidb
    elif augment_en or (mode == 'test' and (cfg.TEST.RAIN_SIM_EN or cfg.TEST.DROPOUT_EN)):
        aug = draw_lidar_augmentation(augment_en=augment_en, mode=mode)
        if not aug.identity:
            if points.shape[0] == 0:
                return [], None, local_roidb
            points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(device, non_blocking=True)
            points, kept = ops.lidar_augment_points(points, aug, aug.seed, expected, out=points)
            if local_roidb is not None:
                augment_gt_boxes(local_roidb[0], aug)
            if int(kept.item()) <= 0:                                                # :428-432
                print('No PC points in frame {} FLIP_X: {} FLIP_Y: {} ROT: {} SWAP_X_Y: {}'.format(
                    filen, aug.flip_x, aug.flip_y, aug.rotation is not None, aug.swap_xy))
                return [], None, local_roidb
    infos, blob = get_lidar_blob(points, scale, device=device, elongation=elongation)
    return [np.asarray(infos[0], dtype=np.float32)], blob, local_roidb


def get_image_minibatch(roidb, num_classes, augment_en, scale, cnt):
    """minibatch.py:180-227: blobs {data, info, gt_boxes (G,5) [x1,y1,x2,y2,cls] scaled, gt_boxes_dc, filename};
    None when the frame has no ground truth left."""
    infos, im_blob, local_roidb = _get_image_blob(roidb, scale, augment_en)
    info, entry = infos[0], local_roidb[0]
    im_scale = info[6]
    gt_inds = np.where(np.asarray(entry['ignore']) == 0)[0]
    gt_boxes = np.empty((len(gt_inds), 5), dtype=np.float32)
    gt_boxes[:, 0:4] = np.asarray(entry['boxes'])[gt_inds, :] * im_scale
    gt_boxes[:, 4] = np.asarray(entry['gt_classes'])[gt_inds]
    dc = np.asarray(entry.get('boxes_dc', np.zeros((0, 4))), dtype=np.float32).reshape(-1, 4)
    gt_boxes_dc = np.empty((dc.shape[0], 5), dtype=np.float32)
    if cfg.TRAIN.IGNORE_DC:
        gt_boxes_dc[:, 0:4] = dc * im_scale
        gt_boxes_dc[:, 4] = 0
    blobs = {'data': im_blob, 'info': info, 'filename': entry['filename'], 'gt_boxes': gt_boxes,
             'gt_boxes_dc': gt_boxes_dc, 'flipped': bool(entry['flipped']) if augment_en else False}
    return blobs if len(gt_boxes) else None


def get_lidar_minibatch(roidb, num_classes, augment_en, scale, cnt):
    """minibatch.py:124-178: gt rows (G,8) [xc,yc,zc,l,w,h,ry,cls] moved onto the voxel grid and scaled."""
    from ..utils.bbox import bbox_pc_to_voxel_grid
    extents = [cfg.LIDAR.X_RANGE[0], cfg.LIDAR.Y_RANGE[0], cfg.LIDAR.Z_RANGE[0],
               cfg.LIDAR.X_RANGE[1], cfg.LIDAR.Y_RANGE[1], cfg.LIDAR.Z_RANGE[1]]
    infos, pc_blob, local_roidb = _get_lidar_blob(roidb, extents, scale, augment_en)
    if pc_blob is None:                                                              # :139-140: go to the next frame
        return None
    info, entry = infos[0], local_roidb[0]
    gt_inds = np.where(np.asarray(entry['ignore']) == 0)[0]
    width = cfg.LIDAR.NUM_BBOX_ELEM + 1
    gt_boxes = np.empty((len(gt_inds), width), dtype=np.float32)
    gt_boxes[:, 0:-1] = bbox_pc_to_voxel_grid(np.array(entry['boxes'], dtype=np.float64)[gt_inds, :], extents, info)
    gt_boxes[:, 0:2] *= scale
    gt_boxes[:, 3:5] *= scale
    gt_boxes[:, -1] = np.asarray(entry['gt_classes'])[gt_inds]
    blobs = {'data': pc_blob, 'flipped': entry['flipped'], 'filename': entry['filename'], 'gt_boxes': gt_boxes,
             'gt_boxes_dc': np.empty(0) * scale, 'info': np.array(info, dtype=np.float32)}
    return blobs if len(gt_boxes) else None


def get_minibatch(roidb, num_classes, augment_en, cnt):
    """minibatch.py:108-122."""
    assert len(roidb) == 1, "Single batch only"
    scale = cfg.TRAIN.SCALES[np.random.randint(0, high=len(cfg.TRAIN.SCALES), size=1)[0]]
    if cfg.NET_TYPE == 'image':
        return get_image_minibatch(roidb, num_classes, augment_en, scale, cnt)
    if cfg.NET_TYPE == 'lidar':
        return get_lidar_minibatch(roidb, num_classes, augment_en, scale, cnt)
    print('getting minibatch failed. Invalid NET TYPE in cfg')
    return None
