"""``test_net(draw_det=True)`` end to end on small frames: one PNG per frame under ``test_drawn/``, its bytes equal to the
restatement's ``render`` of the returned ``all_boxes``, the frame's blob and its ground truth; the records, the graph
pool's counts and the ``draw_det=False`` behaviour untouched by the drawing."""
import os

import numpy as np
import pytest

import draw_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Source:
    """A frame source with the optional members the drawing reads: ``name_at``, ``gt_at``, ``_uncertainty_sort_type``."""
    num_classes = 2
    name = "drawn_frames"

    def __init__(self, blobs, info, gts, sort_type=None):
        self.blobs, self.info, self.gts = blobs, info, gts
        self._uncertainty_sort_type = sort_type

    def num_frames(self, mode):
        return len(self.blobs)

    def blobs_at(self, i, mode):
        return {"data": self.blobs[i], "info": self.info}

    def name_at(self, i, mode):
        return "scene/frame_%d.npy" % i

    def gt_at(self, i, mode):
        return self.gts[i]


def _record_of(all_boxes, i, k, elem, to_grid=None):
    """all_boxes[cls][frame] back into a (K, max_out, E) record the restatement plans from."""
    per_class = [np.zeros((0, elem), np.float32)] + [np.asarray(all_boxes[j][i], np.float32).reshape(-1, elem) for j in range(1, k)]
    max_out = max(1, max(len(r) for r in per_class))
    dets, counts = np.zeros((k, max_out, elem), np.float32), np.zeros(k, np.int32)
    for j in range(1, k):
        rows = per_class[j] if to_grid is None else to_grid(per_class[j])
        dets[j, :len(rows)], counts[j] = rows, len(rows)
    return dets, counts


def _run(test_net, net, src, out, draw, timers):
    return test_net(net, src, out, max_dets=100, thresh=0.01, mode="val", draw_det=draw, timers=timers)


def _assert_same_boxes(a, b):
    for ca, cb in zip(a, b):
        for fa, fb in zip(ca, cb):
            assert fa.shape == fb.shape and np.array_equal(np.asarray(fa).view(np.int32), np.asarray(fb).view(np.int32))


@pytest.mark.parametrize("uc", [False, True])
def test_image_frames_are_drawn(hip, tmp_path, uc):
    """Three 64 x 96 camera frames, ground truth on two of them; with the uncertainty heads the boxes are ordered by
    a_bbox_var (db._uncertainty_sort_type) and their columns travel in the record the plan reads."""
    import torch
    import test_drop_in as D
    from test_draw_host import _read_png
    from faster_rcnn_pytorch_multimodal_amd.model import draw
    from faster_rcnn_pytorch_multimodal_amd.model.test import test_net
    net, _, C = D._image_net(seed=31 if uc else 7, uc=uc)
    try:
        C.cfg.ROOT_DIR = str(tmp_path)
        rng = np.random.default_rng(12)
        info = np.array([0, 96, 0, 64, 0, 0, 1.0], np.float32)
        blobs = [torch.from_numpy((rng.standard_normal((1, 64, 96, 3)) * 60).astype(np.float32)).to(DEV) for _ in range(3)]
        gts = [{"boxes": np.array([[4.5, 6.2, 50.7, 40.1], [30, 10, 90.9, 60]], np.float32), "gt_classes": np.array([1, 0], np.int32)},
               None, {"boxes": np.array([[-3, -2, 200, 30]], np.float32), "gt_classes": np.array([1], np.int32)}]
        src = _Source(blobs, info, gts, sort_type="a_bbox_var" if uc else None)
        folder = draw.draw_folder(src, "test")
        timers = {}
        net.set_uc_seed(5) if uc else None
        plain = _run(test_net, net, src, str(tmp_path / "eval"), False, timers)
        before = dict(timers["pool"])
        assert not os.path.exists(folder)                                   # draw_det=False creates no folder
        os.makedirs(folder)
        open(os.path.join(folder, "stale.png"), "wb").close()
        net.set_uc_seed(5) if uc else None
        drawn = _run(test_net, net, src, str(tmp_path / "eval"), True, timers)
        after = dict(timers["pool"])
        _assert_same_boxes(plain, drawn)
        assert after["captures"] == before["captures"] and after["eager"] == before["eager"] == 0
        assert after["replays"] == before["replays"] + 3
        assert sorted(os.listdir(folder)) == ["img-frame_%d.png" % i for i in range(3)]
        k, elem = 2, 21 if uc else 5
        key = draw.sort_key_columns(src._uncertainty_sort_type, k, False)
        assert (key == (13, 4)) if uc else (key is None)
        total = 0
        for i in range(3):
            dets, counts = _record_of(drawn, i, k, elem)
            total += int(counts.sum())
            gt = gts[i]
            want = R.render(blobs[i].cpu().numpy(), False, dets, counts, gt=None if gt is None else gt["boxes"],
                            gt_labels=None if gt is None else gt["gt_classes"], key=key,
                            stds=C.cfg.PIXEL_STDDEVS.reshape(-1), means=C.cfg.PIXEL_MEANS.reshape(-1),
                            arrange=C.cfg.PIXEL_ARRANGE_BGR)
            got = _read_png(os.path.join(folder, "img-frame_%d.png" % i))
            print("frame %d: %d detections, %d differing bytes" % (i, int(counts.sum()), int((got != want).sum())))
            np.testing.assert_array_equal(got, want)
            bare = R.canvas_image(blobs[i].cpu().numpy(), C.cfg.PIXEL_STDDEVS.reshape(-1), C.cfg.PIXEL_MEANS.reshape(-1),
                                  C.cfg.PIXEL_ARRANGE_BGR)
            assert counts.sum() == 0 or not np.array_equal(got, bare)
        assert total > 0
    finally:
        C.reset_cfg()


def test_lidar_frames_are_drawn(hip, tmp_path):
    """Three 48 x 56 x 15 BEV frames at scale 1.  Points planted inside a ground-truth box light pixels inside its drawn
    footprint: the blob is (y, x, c) and x is the picture's column.  cfg.TEST.DRAW_LIDAR_BOXES=False gives the bare map."""
    import torch
    import test_gpu_parity as T
    from test_draw_host import _read_png
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import draw
    from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device, lidar_extents, test_net
    from faster_rcnn_pytorch_multimodal_amd.utils.bbox import bbox_pc_to_voxel_grid
    net, _ = T._build_lidar_pair(seed=9)
    try:
        C.cfg.ROOT_DIR = str(tmp_path)
        ny, nx = 48, 56
        info = np.array([0, nx, 0, ny, 0, 12, 1.0], np.float32)
        ext = lidar_extents()
        mx, my = (ext[3] - ext[0]) / nx, (ext[4] - ext[1]) / ny            # metres per cell
        # a box 24 cells long in x and 6 wide in y around the point (x 30.25, y 20.25) of the grid, in metres like the roidb's
        gt_box = np.array([[ext[0] + 30.25 * mx, ext[1] + 20.25 * my, 1.0, 24 * mx, 6 * my, 1.5, 0.0]], np.float32)
        gts = [{"boxes": gt_box, "gt_classes": np.array([1], np.int32)}, None,
               {"boxes": np.concatenate([gt_box, gt_box * np.float32([1, 1.5, 1, 0.5, 2, 1, 0]) + np.float32([0, 0, 0, 0, 0, 0, 0.7])]),
                "gt_classes": np.array([0, 1], np.int32)}]
        blobs = []
        for i in range(3):
            b = T._bev_blob(ny, nx, 60 + i)
            b[0, 16:26, 16:46, :] = 0.0
            b[0, 19:22, 20:41, 3] = 0.8                                      # planted points: x 20..40, y 19..21
            b[0, 19:22, 20:41, 12] = 0.5
            blobs.append(torch.from_numpy(b).to(DEV))
        src = _Source(blobs, info, gts)
        folder = draw.draw_folder(src, "test")
        timers = {}
        plain = _run(test_net, net, src, str(tmp_path / "eval"), False, timers)
        before = dict(timers["pool"])
        assert not os.path.exists(folder)
        drawn = _run(test_net, net, src, str(tmp_path / "eval"), True, timers)
        after = dict(timers["pool"])
        _assert_same_boxes(plain, drawn)
        assert after["captures"] == before["captures"] and after["replays"] == before["replays"] + 3 and after["eager"] == 0
        assert sorted(os.listdir(folder)) == ["iter_0_frame_%d.png" % i for i in range(3)]

        def to_grid(rows):
            return bbox_pc_to_voxel_grid(rows.astype(np.float64), ext, info).astype(np.float32) if len(rows) else rows

        total = 0
        for i in range(3):
            dets, counts = _record_of(drawn, i, 2, 8, to_grid)
            total += int(counts.sum())
            gt = gts[i]
            gt_grid = None if gt is None else bbox_pc_to_voxel_grid(gt["boxes"].copy(), ext, info)
            blob = blobs[i].cpu().numpy()
            want = R.render(blob, True, dets, counts, gt=gt_grid, gt_labels=None if gt is None else gt["gt_classes"],
                            bev_form="waymo", slices=12)
            got = _read_png(os.path.join(folder, "iter_0_frame_%d.png" % i))
            print("frame %d: %d detections, %d differing bytes" % (i, int(counts.sum()), int((got != want).sum())))
            np.testing.assert_array_equal(got, want)
            # all_boxes holds metres: the way back to the grid above is not exact in general (the frames are seeded, so the
            # outcome does not vary).  The record itself, as the eager path gives it, has no round trip in it.
            d_dets, d_counts = detect_frame_device(net, blobs[i], info, 0.01, 100, 300)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(got, R.render(blob, True, d_dets.cpu().numpy(), d_counts.cpu().numpy(), gt=gt_grid,
                                                        gt_labels=None if gt is None else gt["gt_classes"],
                                                        bev_form="waymo", slices=12))
            if i == 0:
                # the ground-truth footprint is the only white outline (detections have no red, the map's red stays below
                # 255 / 1.5); the planted cells are the lit ones of the map under it and lie inside it
                white = (got == 255).all(axis=2)
                ys, xs = np.nonzero(white)
                assert (xs.min(), xs.max()) == (18, 43) and (ys.min(), ys.max()) == (17, 24)     # corners 18,17 / 42,23, width 2
                bare = R.canvas_bev(blob, 12, "waymo")[16:26, 16:46, 0] > 0
                assert bare[3:6, 4:25].all() and bare.sum() == 3 * 21
        assert total > 0
        C.cfg.TEST.DRAW_LIDAR_BOXES = False
        _run(test_net, net, src, str(tmp_path / "eval"), True, timers)
        for i in range(3):
            got = _read_png(os.path.join(folder, "iter_0_frame_%d.png" % i))
            np.testing.assert_array_equal(got, R.canvas_bev(blobs[i].cpu().numpy(), 12, "waymo"))
    finally:
        C.reset_cfg()


def test_cold_pool_captures_two_frame_shapes_while_encoders_are_busy(hip, tmp_path, monkeypatch):
    """The reference's own command line: ``test_net(draw_det=True)`` on a pool that has captured nothing, and a second frame
    shape arriving mid-run.  Every encoder thread is held inside ``write_png`` - by a gate the frame source opens when the
    loop asks for its last frame's ground truth, so nothing here sleeps - while the loop captures six graphs; further pictures queue up
    behind them.  Captures are global to the process, so an encoder thread must make no HIP call: the captures succeed (no
    fall-back to eager launches, no warning; the one eager frame is the pool's rule for the first sighting of a further
    shape) and every picture equals the restatement."""
    import threading
    import warnings
    import torch
    import test_drop_in as D
    from test_draw_host import _read_png
    from faster_rcnn_pytorch_multimodal_amd.model import draw
    from faster_rcnn_pytorch_multimodal_amd.model.test import test_net
    net, _, C = D._image_net(seed=7)
    try:
        C.cfg.ROOT_DIR = str(tmp_path)
        rng = np.random.default_rng(21)
        shapes = [(64, 96)] * 4 + [(80, 112), (80, 112), (64, 96), (80, 112)]
        blobs = [torch.from_numpy((rng.standard_normal((1, h, w, 3)) * 60).astype(np.float32)).to(DEV) for h, w in shapes]
        infos = [np.array([0, w, 0, h, 0, 0, 1.0], np.float32) for h, w in shapes]
        gt = {"boxes": np.array([[4.5, 6.2, 50.7, 40.1]], np.float32), "gt_classes": np.array([1], np.int32)}
        gate, held, real_write = threading.Event(), [], draw.write_png

        def gated_write(path, array, level=1):
            held.append(path)
            assert gate.wait(120), "the gate was never opened"
            return real_write(path, array, level)

        class Source(_Source):
            def blobs_at(self, i, mode):
                return {"data": self.blobs[i], "info": self.info[i]}

            def gt_at(self, i, mode):
                if i == len(self.blobs) - 1:
                    gate.set()                                               # asked for after the frame's record is queued:
                return self.gts[i]                                           # every capture is behind the loop now

        monkeypatch.setattr(draw, "write_png", gated_write)
        src = Source(blobs, infos, [gt, None] * 4)
        timers = {}
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            drawn = _run(test_net, net, src, None, True, timers)
        assert not [str(w.message) for w in caught if "EAGERLY" in str(w.message)]
        # lanes 0-3 capture the first shape at first sight; the second shape runs eagerly once, then lanes 1 and 3 capture it
        assert timers["pool"]["captures"] == 6 and timers["pool"]["eager"] == 1 and timers["pool"]["replays"] == 7, timers
        assert not net.frame_pool().uncapturable and len(held) == 8
        folder = draw.draw_folder(src, "test")
        assert sorted(os.listdir(folder)) == ["img-frame_%d.png" % i for i in range(8)]
        for i in range(8):
            dets, counts = _record_of(drawn, i, 2, 5)
            g = src.gts[i]
            want = R.render(blobs[i].cpu().numpy(), False, dets, counts, gt=None if g is None else g["boxes"],
                            gt_labels=None if g is None else g["gt_classes"], stds=C.cfg.PIXEL_STDDEVS.reshape(-1),
                            means=C.cfg.PIXEL_MEANS.reshape(-1), arrange=C.cfg.PIXEL_ARRANGE_BGR)
            np.testing.assert_array_equal(_read_png(os.path.join(folder, "img-frame_%d.png" % i)), want)
    finally:
        C.reset_cfg()
