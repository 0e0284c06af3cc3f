"""Drawing a frame's detections - counterpart of the ``draw_det`` branch of lib/model/test.py:231-242 and of the
``draw_and_save_eval`` it calls (lib/datasets/waymo_imdb.py:190-253, waymo_lidb.py:229-328, kitti_lidb.py:289-378) plus the
folder and file naming of lib/datasets/db.py:192-198,252-258.

The picture is rendered on the device, on the stream that produced the frame's record (``render_frame``: the blob back to
a uint8 canvas, the record to a draw list, the outlines scattered in exact painter's order), copied out as finished bytes
and encoded on the host by ``write_png`` (zlib + struct; Pillow is not a dependency).  ``CanvasRing`` is the bounded
device / pinned-host staging ``test_net(draw_det=True)`` uses.
"""
import os
import shutil
import struct
import time
import zlib

import numpy as np
import torch

from .. import ops
from .config import cfg, get_output_dir

# db.py:283-303: the uncertainties _sort_dets_by_uncertainty can order by, each behind its cfg.UC flag
SORT_KEY_FLAGS = {'a_bbox_var': 'EN_BBOX_ALEATORIC', 'e_bbox_var': 'EN_BBOX_EPISTEMIC', 'a_entropy': 'EN_CLS_ALEATORIC',
                  'a_mutual_info': 'EN_CLS_ALEATORIC', 'a_cls_var': 'EN_CLS_ALEATORIC', 'e_mutual_info': 'EN_CLS_EPISTEMIC',
                  'e_entropy': 'EN_CLS_EPISTEMIC'}
LIMITER = 15                           # waymo_imdb.py:208, waymo_lidb.py:265
# pinned host memory test_net(draw_det=True) may hold in finished canvases waiting for their encoder
HOST_RING_BYTES = 256 << 20
ENCODE_THREADS = 8


def sort_key_columns(sort_key, num_classes, lidar):
    """``(first column, column count)`` of uncertainty ``sort_key`` in a detection row [box, score, uncertainty columns in
    nets.uncertainty.UNCERTAINTY_ORDER], or None when the reference would fall back to the row order (db.py:298-299: the
    key is not one it knows, or its cfg.UC flag is off)."""
    from ..nets.uncertainty import UNCERTAINTY_ORDER
    if sort_key is None or sort_key not in SORT_KEY_FLAGS or not cfg.UC[SORT_KEY_FLAGS[sort_key]]:
        return None
    elem = 7 if lidar else 4
    col = elem + 1
    for name in UNCERTAINTY_ORDER:
        if name.endswith('bbox_var'):
            on, width = cfg.UC['EN_BBOX_ALEATORIC' if name[0] == 'a' else 'EN_BBOX_EPISTEMIC'], elem
        else:
            on = cfg.UC['EN_CLS_ALEATORIC' if name[0] == 'a' else 'EN_CLS_EPISTEMIC']
            width = num_classes if name.endswith('cls_var') else 1
        if not on:
            continue
        if name == sort_key:
            return col, width
        col += width
    return None


def bev_form():
    """Which BEV colouring the reference's dataset class of cfg.DB_NAME uses: waymo_lidb.py:240-261, or
    kitti_lidb.py:289-297 for KITTI and CADC."""
    return 'kitti' if str(cfg.DB_NAME).lower() in ('kitti', 'cadc') else 'waymo'


def gt_arrays(gt, info, lidar):
    """A frame's ground truth ({'boxes', 'gt_classes'} or None) as the host arrays the plan takes: float32 (G, 4 or 7) and
    int32 (G,), or None without boxes.  LiDAR boxes go from metres to the voxel grid like lib/model/test.py:238-239 (on a
    copy: the reference converts the roidb's rows in place)."""
    if gt is None or gt.get('boxes') is None or len(gt['boxes']) == 0:
        return None
    boxes = np.array(gt['boxes'], dtype=np.float32, copy=True)
    if lidar:
        from ..utils.bbox import bbox_pc_to_voxel_grid
        from .test import lidar_extents
        boxes = bbox_pc_to_voxel_grid(boxes, lidar_extents(), info)
    boxes = np.ascontiguousarray(boxes[:, :7 if lidar else 4], dtype=np.float32)
    return boxes, np.ascontiguousarray(gt['gt_classes'], dtype=np.int32)


def upload_gt(gt, info, lidar, device):
    """``gt_arrays`` as the ``(boxes, labels)`` device tensors ``render_frame`` takes, or None."""
    arrays = gt_arrays(gt, info, lidar)
    return None if arrays is None else tuple(torch.from_numpy(a).to(device) for a in arrays)


def render_frame(blob, info, dets, counts, gt=None, sort_key=None, out=None, scratch=None):
    """One frame's picture on the device, all launches on the current stream, no host synchronisation.
    ``blob``: the frame's (1, H, W, 3) image blob or (1, Ny, Nx, C) BEV blob (cfg.NET_TYPE decides); ``dets`` (K, max_out, E)
    / ``counts`` (K,) as ``detect_frame_device`` or a ``FrameRunner`` returns them, uncertainty columns included;
    ``gt``: None or the ``(boxes, labels)`` device tensors of ``upload_gt``; ``sort_key``: the uncertainty that orders a
    class's detections (``db._uncertainty_sort_type``).  Returns the (H, W, 3) uint8 device canvas (``out`` or a new one).
    ``info`` is the frame's 7-vector (unused by the drawing itself: the record is in blob coordinates already).
    cfg.TEST.DRAW_LIDAR_BOXES False: a LiDAR frame is its BEV map alone (the reference's literal picture)."""
    lidar = cfg.NET_TYPE == 'lidar'
    scratch = scratch if scratch is not None else {}
    if lidar:
        canvas = ops.canvas_from_bev_blob(blob, bev_form(), out=out, ws=scratch.get('ws'))
        if not cfg.TEST.DRAW_LIDAR_BOXES:
            return canvas
    else:
        canvas = ops.canvas_from_image_blob(blob, out=out)
    k = int(dets.shape[0])
    boxes, labels = gt if gt is not None else (None, None)
    rows = ops.draw_plan(dets, counts, canvas.shape[:2], lidar, key=sort_key_columns(sort_key, k, lidar), limiter0=LIMITER,
                         gt=boxes, gt_labels=labels)
    owner = scratch.get('owner')
    if owner is not None and tuple(owner.shape) != tuple(canvas.shape[:2]):
        owner = None
    return ops.draw_boxes(canvas, rows, owner=owner)


def _chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, array, level=1):
    """``array`` (H, W, 3) uint8 -> an 8-bit RGB PNG, every scanline with filter 0, written with zlib and struct alone."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: expected a (H, W, 3) uint8 array, got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + w * 3), np.uint8)           # filter byte 0 in front of every scanline
    raw[:, 1:] = a.reshape(h, w * 3)
    data = (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
            + _chunk(b'IDAT', zlib.compress(raw.tobytes(), level)) + _chunk(b'IEND', b''))
    with open(path, 'wb') as f:
        f.write(data)
    return path


def draw_folder(db, mode='test'):
    """<get_output_dir(db, 'test')>/test_drawn (db.py:252-258 with lib/model/test.py:175's test_mode)."""
    return os.path.join(get_output_dir(db, mode=mode), '%s_drawn' % mode)


def reset_draw_folder(db, mode='test'):
    """db.delete_eval_draw_folder (db.py:192-198, called at lib/model/test.py:176): the folder is emptied at the start of a
    run."""
    path = draw_folder(db, mode)
    if os.path.isdir(path):
        shutil.rmtree(path)
    os.makedirs(path)
    return path


def frame_file_name(frame_name, lidar):
    """waymo_imdb.py:193-195 with iter 0 ('img-<basename>.png') / waymo_lidb.py:231 ('iter_0_<basename>.png'): the basename
    of the frame's file with its extension replaced."""
    base = os.path.basename(str(frame_name))
    stem = os.path.splitext(base)[0] if '.' in base else base
    return ('iter_0_%s.png' if lidar else 'img-%s.png') % stem


def _encode(ring, slot, ticket, path, view):
    """An encoder thread's task: wait until the picture's ticket has arrived in pinned memory, then write the file.
    The wait reads host memory only.  A worker thread must make no HIP call: frames are captured into graphs on the loop's
    thread while encoders run (``FramePool.runner``), a capture is global to the process, and a runtime call from another
    thread while it lasts can invalidate it (``frame_graph.capture``)."""
    while ring.tickets[slot] != ticket:
        if ring.abort:
            return None
        time.sleep(0.0005)
    return write_png(path, view)


class CanvasRing:
    """Bounded staging of ``test_net(draw_det=True)``'s pictures.

    Device side: one canvas, one owner plane, one BEV workspace and one ticket word per lane (frame s renders into lane
    s % lanes on that lane's stream, behind the copy-out of the lane's previous picture: stream order is the only
    dependency) = lanes * 7 * H * W bytes + the draw lists.  Host side: pinned canvases of H * W * 3 bytes, at most
    ``HOST_RING_BYTES`` of them (never fewer than ``lanes``), and one pinned ticket word per slot.  Behind a picture's copy
    the lane's stream copies the frame's number into the slot's ticket word; the picture's encoder task is queued with the
    frame and watches that word from its own thread, so pictures are encoded as they finish, while the loop queues and the
    device runs the frames behind them.  Neither the queueing loop nor an encoder waits in the HIP runtime.  A slot is
    reused only after its file is written: while the ring holds every frame the loop keeps in flight that is never a
    wait; a frame so large that it does not (1280x1920: 7.4 MB a canvas, 36 slots for 2 x 64 queued frames) makes the loop
    wait for the encoder of the frame queued 36 frames earlier - for the encoders, the actual bound, not for the device to
    drain."""

    def __init__(self, folder, lanes, device, lidar, threads=ENCODE_THREADS):
        from concurrent.futures import ThreadPoolExecutor
        self.folder, self.lanes, self.device, self.lidar = folder, max(1, int(lanes)), device, lidar
        self.dev = [dict() for _ in range(self.lanes)]
        self.host, self.busy = [], []              # per slot: pinned canvas; the Future of its encoder task or None
        self.gt_host = []                          # per slot: pinned staging of the frame's ground truth
        self.tickets_pinned, self.tickets = None, None     # per slot: frame number + 1 once its picture is on the host
        self.abort = False
        self.count = 0
        self.encoders = ThreadPoolExecutor(max_workers=threads)

    def _slots_for(self, nbytes):
        return max(self.lanes, HOST_RING_BYTES // max(nbytes, 1))

    def _release(self, slot):
        if self.busy[slot] is not None:
            self.busy[slot].result()               # re-raises what the encoder raised
            self.busy[slot] = None

    def _upload_gt(self, slot, gt, info):
        """The frame's ground truth through the slot's own pinned staging buffer: no allocation per frame, and no wait
        for the stream, which a copy from pageable memory would bring."""
        arrays = gt_arrays(gt, info, self.lidar)
        if arrays is None:
            return None
        boxes, labels = arrays
        nb, nl = boxes.size * 4, labels.size * 4
        if self.gt_host[slot] is None or self.gt_host[slot].numel() < nb + nl:
            self.gt_host[slot] = torch.empty(max(nb + nl, 4096), dtype=torch.uint8, pin_memory=True)
        hb = self.gt_host[slot][:nb].view(torch.float32).view(boxes.shape)
        hl = self.gt_host[slot][nb:nb + nl].view(torch.int32)
        hb.copy_(torch.from_numpy(boxes))
        hl.copy_(torch.from_numpy(labels))
        return hb.to(self.device, non_blocking=True), hl.to(self.device, non_blocking=True)

    def render(self, lane, blob, info, dets, counts, gt, sort_key, frame_name):
        """Queue one frame's picture on the current stream (the lane's), its copy to pinned memory, its ticket and its
        encoder task.  ``gt``: the frame source's {'boxes', 'gt_classes'} or None."""
        h, w = int(blob.shape[1]), int(blob.shape[2])
        nbytes = h * w * 3
        d = self.dev[lane]
        if d.get('hw') != (h, w):
            d['hw'] = (h, w)
            d['canvas'] = torch.empty((h, w, 3), dtype=torch.uint8, device=self.device)
            d['owner'] = torch.empty((h, w), dtype=torch.int32, device=self.device)
            d['ws'] = ops.canvas_bev_workspace(self.device) if self.lidar else None
        if 'ticket' not in d:
            d['ticket'] = torch.zeros(1, dtype=torch.int64, device=self.device)
        if not self.host:
            n = self._slots_for(nbytes)
            self.host, self.busy, self.gt_host = [None] * n, [None] * n, [None] * n
            self.tickets_pinned = torch.zeros(n, dtype=torch.int64, pin_memory=True)
            self.tickets = self.tickets_pinned.numpy()
        slot, ticket = self.count % len(self.host), self.count + 1
        self.count += 1
        self._release(slot)
        canvas = render_frame(blob, info, dets, counts, gt=self._upload_gt(slot, gt, info), sort_key=sort_key,
                              out=d['canvas'], scratch=d)
        if self.host[slot] is None or self.host[slot].numel() < nbytes:
            self.host[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        view = self.host[slot][:nbytes].view(h, w, 3)
        view.copy_(canvas, non_blocking=True)
        d['ticket'].fill_(ticket)                  # stream order: the ticket lands after the last byte of the picture
        self.tickets_pinned[slot:slot + 1].copy_(d['ticket'], non_blocking=True)
        path = os.path.join(self.folder, frame_file_name(frame_name, self.lidar))
        self.busy[slot] = self.encoders.submit(_encode, self, slot, ticket, path, view.numpy())

    def close(self, abort=False):
        """Every picture is on disk when this returns.  ``abort``: the loop failed - the encoders stop waiting for
        pictures that may never come, and their own errors are dropped in favour of the loop's."""
        self.abort = bool(abort)
        try:
            if not abort:
                for slot in range(len(self.busy)):
                    self._release(slot)
        finally:
            self.abort = True
            self.encoders.shutdown(wait=True)
