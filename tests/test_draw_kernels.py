"""The drawing kernels (csrc/draw.hip) against tests/draw_restatement.py, bit for bit, every output between guard bands:
the two canvas producers, the draw plan (order, colours, geometry) and the scatter / compose painter.  Nothing here has a
tolerance: every byte is decided in float64 or integer arithmetic on both sides."""
import numpy as np
import pytest
import torch

import draw_restatement as R
from guarded_buffers import DEV, GUARD, guarded

pytestmark = pytest.mark.gpu

UC_FLAGS = ("EN_BBOX_ALEATORIC", "EN_CLS_ALEATORIC", "EN_BBOX_EPISTEMIC", "EN_CLS_EPISTEMIC")
KEYS = (None, 'a_bbox_var', 'e_bbox_var', 'a_entropy', 'a_mutual_info', 'a_cls_var', 'e_mutual_info', 'e_entropy')


class Guarded:
    """An output of ``shape`` / ``dtype`` in the middle of a NaN-filled allocation; ``intact()``: no byte outside the
    output changed (the bands and the up to three slack bytes behind an odd-sized output)."""

    def __init__(self, shape, dtype, fill=0xA5):
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(shape)) * item
        self.buf, _ = guarded((self.nbytes + 3) // 4)
        self.bytes = self.buf.view(torch.uint8)
        self.lo = GUARD * 4
        region = self.bytes[self.lo:self.lo + self.nbytes]
        region.fill_(fill)
        self.view = region.view(dtype).view(*shape)
        self.before = self.bytes.clone()

    def intact(self):
        after = self.bytes.clone()
        after[self.lo:self.lo + self.nbytes] = self.before[self.lo:self.lo + self.nbytes]
        return torch.equal(after, self.before)


def _ops():
    from faster_rcnn_pytorch_multimodal_amd import ops
    return ops


@pytest.fixture
def cfg():
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    C.reset_cfg()
    yield C.cfg
    C.reset_cfg()


# ---------------------------------------------------------------------------------------------------------------------
# canvases

@pytest.mark.parametrize("h,w", [(5, 7), (33, 65)])
def test_image_canvas_is_bit_equal(hip, cfg, h, w):
    """waymo_imdb.py:200-204: values below 0, above 255, exactly on integers (with 254.99999 -> 254), NaN and +-Inf, with
    non-unit PIXEL_STDDEVS and the BGR channel order."""
    rng = np.random.default_rng(h)
    cfg.PIXEL_STDDEVS = np.array([[[57.375, 1.0, 0.5]]])
    cfg.PIXEL_MEANS = np.array([[[96.866, 98.0, 93.85]]])
    blob = (rng.standard_normal((1, h, w, 3)) * 3).astype(np.float32)
    blob[0, :, :, 1] = rng.integers(-120, 180, (h, w))                        # + 98.0: exactly on integers, some outside [0, 255]
    blob[0, 0, 0] = [np.nan, np.inf, -np.inf]
    blob[0, 1, 1] = [-50.0, 157.0, 1000.0]
    blob[0, 2, 2, 1] = np.float32(254.99999 - 98.0)
    blob[0, 3, 3, 1] = 255.0 - 98.0
    want = R.canvas_image(blob, cfg.PIXEL_STDDEVS.reshape(-1), cfg.PIXEL_MEANS.reshape(-1), cfg.PIXEL_ARRANGE_BGR)
    assert want[2, 2, 1] == 254 and want[3, 3, 1] == 255 and want.min() == 0 and want.max() == 255
    assert list(want[0, 0]) == [0, 255, 0]                                    # BGR -> RGB: (-Inf, +Inf, NaN) saturated
    out = Guarded((h, w, 3), torch.uint8)
    dev = torch.from_numpy(blob).to(DEV)
    got = _ops().canvas_from_image_blob(dev, out=out.view)
    torch.cuda.synchronize()
    assert out.intact()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(_ops().canvas_from_image_blob(dev).cpu().numpy(), want)


def _bev_blob(ny, nx, kind, seed):
    rng = np.random.default_rng(seed)
    blob = np.zeros((1, ny, nx, 15), np.float32)
    if kind == "empty":
        return blob
    if kind == "one_cell":
        blob[0, ny // 2, nx // 3, 4] = 1.25
        blob[0, ny // 2, nx // 3, 12:15] = [0.4, 0.7, 1.0]
        return blob
    occupied = rng.random((ny, nx)) < 0.4
    heights = (rng.random((ny, nx, 12)) * 3.0).astype(np.float32) * (rng.random((ny, nx, 12)) < 0.3)
    if kind == "negative":
        heights = heights - np.float32(1.5) * (heights != 0)               # negative heights, |v| straddling 1e-5
        heights[0, 0, 0] = 5e-6
    blob[0, :, :, :12] = heights * occupied[:, :, None]
    blob[0, :, :, 12] = 0.0 if kind == "no_density" else rng.random((ny, nx)) * occupied
    blob[0, :, :, 13] = rng.random((ny, nx)) * occupied * 7.0
    blob[0, :, :, 14] = 1.0
    return blob


@pytest.mark.parametrize("form", ["waymo", "kitti"])
@pytest.mark.parametrize("ny,nx", [(9, 11), (70, 66)])
@pytest.mark.parametrize("kind", ["dense", "negative", "no_density", "one_cell", "empty"])
def test_bev_canvas_is_bit_equal_and_leaves_the_blob_alone(hip, cfg, form, ny, nx, kind):
    """waymo_lidb.py:240-261 / kitti_lidb.py:289-297: 70 x 66 cells need more than one workgroup's partial; an empty grid, a
    single occupied cell and a density maximum of 0 are the empty ranges the reference divides by."""
    blob = _bev_blob(ny, nx, kind, ny + len(kind))
    want = R.canvas_bev(blob, 12, form)
    if kind == "dense":
        assert want[:, :, 0].max() > 100 and want[:, :, 1].max() >= 254
    if kind in ("empty", "no_density"):
        assert want[:, :, 1].max() == 0
    dev = torch.from_numpy(blob).to(DEV)
    out = Guarded((ny, nx, 3), torch.uint8)
    ws = Guarded((int(hip.frcnn_canvas_from_bev_blob_ws_bytes()),), torch.uint8)
    got = _ops().canvas_from_bev_blob(dev, form, out=out.view, ws=ws.view)
    torch.cuda.synchronize()
    assert out.intact() and ws.intact()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.int32), blob.view(np.int32))     # the input blob is unchanged


# ---------------------------------------------------------------------------------------------------------------------
# plan

def _record(k, max_out, counts, lidar, seed):
    """A record with every uncertainty column: finite keys with planted ties, boxes over and beyond the canvas."""
    from faster_rcnn_pytorch_multimodal_amd.nets.uncertainty import num_uncertainty_pos
    rng = np.random.default_rng(seed)
    box = 7 if lidar else 4
    elem = box + 1 + num_uncertainty_pos(k, box)
    dets = np.zeros((k, max_out, elem), np.float32)
    if lidar:
        dets[:, :, 0] = rng.uniform(-5, 60, (k, max_out))
        dets[:, :, 1] = rng.uniform(-5, 70, (k, max_out))
        dets[:, :, 3:6] = rng.uniform(0.5, 20, (k, max_out, 3))
        dets[:, :, 6] = rng.uniform(-np.pi, np.pi, (k, max_out))
        dets[:, :4, 6] = [0.3, 2.0, -2.5, -0.4]                               # ry in all four quadrants
        dets[:, 4, 6] = 0.0
    else:
        x0, y0 = rng.uniform(-20, 90, (k, max_out)), rng.uniform(-20, 60, (k, max_out))
        dets[:, :, 0], dets[:, :, 1] = x0, y0
        dets[:, :, 2], dets[:, :, 3] = x0 + rng.uniform(0, 50, (k, max_out)), y0 + rng.uniform(0, 40, (k, max_out))
    dets[:, :, box] = rng.uniform(0.0, 1.0, (k, max_out))
    dets[:, 0, box] = 1.0
    unc = rng.uniform(0.0, 2.0, (k, max_out, elem - box - 1)).astype(np.float32)
    unc[:, 5] = unc[:, 2]                                                       # planted ties: rows 2, 5 and 9 share every key
    unc[:, 9] = unc[:, 2]
    dets[:, :, box + 1:] = unc
    if max_out > 12:
        dets[1, 3, 0 if lidar else 2] = np.nan                                  # a NaN coordinate: the row is skipped
    return dets, np.asarray(counts, np.int32)


PLAN_COUNTS = [(2, (0, 0)), (2, (9, 1)), (2, (0, 15)), (2, (0, 16)), (2, (0, 40)), (5, (3, 1, 15, 16, 40)),
               (5, (0, 40, 0, 16, 15)), (5, (0, 16, 40, 1, 0))]


@pytest.mark.parametrize("lidar", [False, True])
@pytest.mark.parametrize("k,counts", PLAN_COUNTS)
def test_plan_equals_the_restatement_row_for_row(hip, cfg, lidar, k, counts):
    """Counts of 0, 1, 15, 16 and 40 make ``limiter`` switch and ``uc_gradient`` go negative; every uncertainty key and
    none; ties, a NaN coordinate, ground truth of both labels; LiDAR footprints in all four quadrants."""
    from faster_rcnn_pytorch_multimodal_amd.model.draw import sort_key_columns
    for flag in UC_FLAGS:
        cfg.UC[flag] = True
    max_out, hw = 40, (64, 96)
    dets, cnt = _record(k, max_out, counts, lidar, seed=k + sum(counts))
    rng = np.random.default_rng(11)
    if lidar:
        gt = np.concatenate([rng.uniform(0, 60, (5, 3)), rng.uniform(1, 15, (5, 3)), rng.uniform(-3, 3, (5, 1))], 1).astype(np.float32)
    else:
        gt = np.concatenate([rng.uniform(-5, 40, (5, 2)), rng.uniform(40, 110, (5, 2))], 1).astype(np.float32)
    gt[3, 1] = np.nan
    labels = np.array([1, 0, 2, 1, 0], np.int32)
    d_dets, d_cnt = torch.from_numpy(dets).to(DEV), torch.from_numpy(cnt).to(DEV)
    d_gt, d_lab = torch.from_numpy(gt).to(DEV), torch.from_numpy(labels).to(DEV)
    blues = set()
    for name in KEYS:
        key = sort_key_columns(name, k, lidar)
        assert (key is None) == (name is None)
        for with_gt in (True, False):
            want = R.plan(dets, cnt, hw, lidar, key=key, gt=gt if with_gt else None, gt_labels=labels if with_gt else None)
            out = Guarded(want.shape, torch.int32)
            got = _ops().draw_plan(d_dets, d_cnt, hw, lidar, key=key, gt=d_gt if with_gt else None,
                                   gt_labels=d_lab if with_gt else None, rows=out.view)
            torch.cuda.synchronize()
            assert out.intact()
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg="%s gt=%s" % (name, with_gt))
        blues |= set(((want[:, 3] >> 16) & 255).tolist())
    n = int(sum(min(c, max_out) for c in counts[1:]))
    assert (want[:n, 0] != R.SKIP).sum() >= n - 1 and not want[n:, 0].any()
    if max(counts[1:]) == 40:
        assert 0 in blues and 255 in blues                                      # (limiter - i) / limiter < 0 was clamped


# ---------------------------------------------------------------------------------------------------------------------
# scatter / compose

H, W = 40, 48


def _rect(x0, y0, x1, y1, wd, rgb):
    return [R.RECT, wd, 0, rgb, x0, y0, x1, y1, 0, 0, 0, 0]


def _rows(items):
    rows = np.asarray(items, np.int32).reshape(-1, R.ROW_INTS)
    rows[:, 2] = np.arange(len(rows))
    return rows


def _random_rows(n, seed):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n):
        rgb = int(rng.integers(1, 1 << 24))
        kind = rng.integers(0, 8)
        wd = int(rng.integers(1, 4))
        if kind == 0:
            items.append([R.SKIP, wd, 0, rgb] + [int(v) for v in rng.integers(0, 40, 8)])
        elif kind < 5:
            x0, y0 = int(rng.integers(-12, W + 4)), int(rng.integers(-12, H + 4))
            items.append(_rect(x0, y0, x0 + int(rng.integers(-2, 30)), y0 + int(rng.integers(-2, 30)), wd, rgb))
        else:
            pts = [int(v) for pair in zip(rng.integers(-4, W + 4, 4), rng.integers(-4, H + 4, 4)) for v in pair]
            items.append([R.FOOTPRINT, min(wd, 2), 0, rgb] + pts)
    return _rows(items)


SCATTER_CASES = {
    "none": _rows([]),
    "one_pixel": _rows([_rect(7, 9, 7, 9, 2, 0x0000FF), _rect(0, 0, 0, 0, 1, 0x00FF00), _rect(W - 1, H - 1, W - 1, H - 1, 3, 0xFF0000)]),
    "borders": _rows([_rect(0, 0, W - 1, H - 1, 2, 0x112233), _rect(-5, 5, 10, 12, 2, 0x445566), _rect(40, -3, 60, 8, 2, 0x778899),
                      _rect(-9, 30, 70, 50, 1, 0xAABBCC), _rect(20, 36, 30, 39, 2, 0xDDEEFF), _rect(-50, -50, 200, 200, 2, 0x010203),
                      _rect(W, 3, W + 9, 9, 2, 0x0A0B0C), _rect(-9, -9, -1, -1, 2, 0x0D0E0F), _rect(46, 2, 47, 30, 1, 0x123456),
                      [R.FOOTPRINT, 2, 0, 0x654321, 0, 0, W - 1, 0, W - 1, H - 1, 0, H - 1]]),
    "thin": _rows([_rect(3, 3, 5, 20, 2, 0x0000FF), _rect(10, 10, 30, 12, 2, 0x00FF00), _rect(12, 20, 12, 35, 1, 0xFF0000),
                   _rect(20, 20, 22, 22, 2, 0x00FFFF), _rect(30, 5, 29, 9, 2, 0xFFFFFF), _rect(33, 5, 36, 8, 3, 0xFF00FF)]),
    "random300": _random_rows(300, 4),
}


@pytest.mark.parametrize("case", sorted(SCATTER_CASES))
def test_painter_equals_the_serial_painter(hip, case):
    """Exact painter's order on a 40 x 48 canvas: where outlines cross the later row wins, and two runs give the same bytes."""
    rows = SCATTER_CASES[case]
    base = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    want = R.paint(base, rows)
    if case == "none":
        assert np.array_equal(want, base)
    else:
        assert not np.array_equal(want, base)
    d_rows = torch.from_numpy(rows.copy()).to(DEV)
    runs = []
    for _ in range(2):
        canvas, owner = Guarded((H, W, 3), torch.uint8), Guarded((H, W), torch.int32)
        canvas.view.copy_(torch.from_numpy(base).to(DEV))
        got = _ops().draw_boxes(canvas.view, d_rows, owner=owner.view)
        torch.cuda.synchronize()
        assert canvas.intact() and owner.intact()
        runs.append(got.cpu().numpy())
    np.testing.assert_array_equal(runs[0], want)
    np.testing.assert_array_equal(runs[1], runs[0])


def test_a_captured_render_holds_kernel_nodes_only(hip, cfg):
    """canvas + plan + scatter (with its clear) + compose captured on a stream: kernel nodes only, replay == eager."""
    from faster_rcnn_pytorch_multimodal_amd.model.draw import render_frame
    from faster_rcnn_pytorch_multimodal_amd.model.train_graph import graph_node_kinds
    cfg.NET_TYPE = "image"
    dets, cnt = _record(2, 40, (0, 40), False, seed=8)
    d_dets, d_cnt = torch.from_numpy(dets[:, :, :5].copy()).to(DEV), torch.from_numpy(cnt).to(DEV)
    blob = torch.from_numpy((np.random.default_rng(2).standard_normal((1, 64, 96, 3)) * 60).astype(np.float32)).to(DEV)
    info = np.array([0, 96, 0, 64, 0, 0, 1.0], np.float32)
    gt = (torch.tensor([[5.0, 6.0, 50.0, 40.0]], device=DEV), torch.tensor([1], dtype=torch.int32, device=DEV))
    eager = render_frame(blob, info, d_dets, d_cnt, gt=gt).cpu().numpy()
    want = R.render(blob.cpu().numpy(), False, dets[:, :, :5], cnt, gt=gt[0].cpu().numpy(), gt_labels=[1],
                    means=cfg.PIXEL_MEANS.reshape(-1))
    np.testing.assert_array_equal(eager, want)
    out = torch.empty((64, 96, 3), dtype=torch.uint8, device=DEV)
    scratch = {"owner": torch.empty((64, 96), dtype=torch.int32, device=DEV)}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        render_frame(blob, info, d_dets, d_cnt, gt=gt, out=out, scratch=scratch)
    kinds, nodes, _ = graph_node_kinds(graph)
    assert set(kinds) == {"kernel"} and nodes == kinds["kernel"] == 5, kinds     # canvas, plan, clear, scatter, compose
    graph.instantiate()
    for _ in range(2):
        out.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), eager)


def test_rejections(hip, cfg):
    from faster_rcnn_pytorch_multimodal_amd import _hip
    ops = _ops()
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    for call in (lambda: ops.canvas_from_image_blob(z(1, 4, 4, 4)),
                 lambda: ops.canvas_from_image_blob(z(1, 4, 4, 3), out=z(4, 4, 3)),
                 lambda: ops.canvas_from_bev_blob(z(1, 4, 4, 15), "nuscenes"),
                 lambda: ops.canvas_from_bev_blob(z(1, 4, 4, 13), "waymo"),
                 lambda: ops.draw_plan(z(2, 5, 4), z(2, dtype=torch.int32), (8, 8), False),
                 lambda: ops.draw_plan(z(2, 5, 5), z(2, dtype=torch.int32), (8, 8), False, key=(4, 2)),
                 lambda: ops.draw_plan(z(2, 5000, 5), z(2, dtype=torch.int32), (8, 8), False),
                 lambda: ops.draw_plan(z(2, 5, 8), z(2, dtype=torch.int32), (8, 8), True, gt=z(3, 4), gt_labels=z(3, dtype=torch.int32)),
                 lambda: ops.draw_boxes(z(8, 8, 3, dtype=torch.uint8), z(2, 11, dtype=torch.int32)),
                 lambda: ops.draw_boxes(z(8, 8, 3), z(2, 12, dtype=torch.int32))):
        with pytest.raises(_hip.HipError):
            call()
