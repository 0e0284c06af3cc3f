"""Host side of the detection drawing (model/draw.py, tests/draw_restatement.py): the restated outline and edge rules
against Pillow, the stdlib PNG writer, the reference's file names and folders, and ``gt_at`` through ``ReferenceDb``.
No GPU."""
import os
import struct
import zlib

import numpy as np
import pytest

import draw_restatement as R


def _pillow_rect(corners, outline, wd, height, width):
    from PIL import Image, ImageDraw
    im = Image.new('RGB', (width, height), (9, 9, 9))
    ImageDraw.Draw(im).rectangle([(corners[0], corners[1]), (corners[2], corners[3])], outline=outline, width=wd)
    return np.array(im)


# float, negative and beyond-canvas corners; every case has x1 - x0 >= 2w and y1 - y0 >= 2w after Pillow's conversion
RECT_CASES = [
    (3, 4, 20, 15), (3.9, 4.2, 20.99, 15.5), (0, 0, 47, 39), (-3.7, 2.9, 8.99, 30.2), (-10.5, -7.2, 4.4, 5.1),
    (30.2, 25.7, 60.0, 90.5), (-5, -5, 100, 100), (-0.9, -0.9, 4.1, 4.9), (10, -20.5, 14.2, 70), (43.5, 35.2, 47.9, 39.9),
    (-30, 10, -20, 30), (60, 5, 75, 20), (5, 5, 9, 9), (1e6, 2, 1e6 + 8, 30), (-1e6, -1e6, 1e6, 1e6), (46, 10, 1e9, 20),
]


@pytest.mark.parametrize("wd", [1, 2])
def test_outline_rule_equals_pillow_rectangle(wd):
    """The restated rule (pixels of the inclusive integer box within w of its border, corners truncated toward zero) is
    Pillow's ImageDraw.rectangle(outline=, width=w) on the domain x1 - x0 >= 2w, y1 - y0 >= 2w."""
    pytest.importorskip("PIL")
    height, width = 40, 48
    for case in RECT_CASES:
        g = [R.pil_int(v) for v in case]
        assert g[2] - g[0] >= 2 * wd and g[3] - g[1] >= 2 * wd, case
        want = _pillow_rect(case, (10, 200, 30), wd, height, width)
        got = np.full((height, width, 3), 9, np.uint8)
        got[R.rect_mask(g[0], g[1], g[2], g[3], wd, height, width)] = (10, 200, 30)
        np.testing.assert_array_equal(got, want, err_msg=str(case))


def test_colours_are_clamped_like_pillow():
    pytest.importorskip("PIL")
    for colour in [(0, 300, -5), (256, 255, 0), (-1, 1000, 128)]:
        want = _pillow_rect((2, 2, 12, 12), colour, 2, 16, 16)
        assert tuple(want[2, 2]) == tuple(R.clamp255(c) for c in colour)


def _pillow_line(a, b, height, width):
    from PIL import Image, ImageDraw
    im = Image.new('L', (width, height), 0)
    ImageDraw.Draw(im).line([a[0], a[1], b[0], b[1]], fill=255, width=1)
    return np.array(im) > 0


def test_edge_rule_equals_pillow_line_in_every_octant():
    """Width-1 edges: the closed form equals Pillow's Bresenham walk pixel for pixel - all eight octants with both tie
    parities, the diagonals, horizontal, vertical and zero length, from either end."""
    pytest.importorskip("PIL")
    height, width = 40, 48
    c = (20, 18)
    ends = []
    for dx, dy in [(17, 5), (17, 6), (5, 17), (6, 17), (12, 12), (16, 8), (8, 16), (15, 0), (0, 15), (0, 0), (1, 1), (2, 1),
                   (1, 2), (3, 2), (19, 1), (1, 17)]:
        for sx in (1, -1):
            for sy in (1, -1):
                ends.append((c[0] + sx * dx, c[1] + sy * dy))
    rng = np.random.default_rng(3)
    pairs = [(c, e) for e in ends] + [(e, c) for e in ends]
    pairs += [((int(a), int(b)), (int(p), int(q))) for a, b, p, q in zip(rng.integers(0, width, 400), rng.integers(0, height, 400),
                                                                          rng.integers(0, width, 400), rng.integers(0, height, 400))]
    for a, b in pairs:
        want = _pillow_line(a, b, height, width)
        got = R.edge_mask(a[0], a[1], b[0], b[1], 1, height, width)
        np.testing.assert_array_equal(got, want, err_msg="%s -> %s" % (a, b))


def test_width_two_edge_adds_the_minor_axis_neighbour():
    one = R.edge_mask(2, 3, 12, 7, 1, 16, 16)
    two = R.edge_mask(2, 3, 12, 7, 2, 16, 16)
    assert np.array_equal(two, one | np.roll(one, 1, axis=0))            # x-major: the neighbour at y + 1
    one = R.edge_mask(5, 1, 7, 15, 1, 16, 16)
    two = R.edge_mask(5, 1, 7, 15, 2, 16, 16)
    want = one.copy()
    want[:, 1:] |= one[:, :-1]                                            # y-major: the neighbour at x + 1
    assert np.array_equal(two, want)
    assert R.edge_mask(15, 2, 15, 9, 2, 16, 16).sum() == 8               # the neighbour column 16 is off the canvas


def test_serial_painter_later_rows_win():
    rows = np.zeros((3, R.ROW_INTS), np.int32)
    rows[0] = [R.RECT, 2, 0, 0x0000FF, 1, 1, 10, 10, 0, 0, 0, 0]
    rows[1] = [R.RECT, 1, 1, 0x00FF00, 5, 0, 14, 8, 0, 0, 0, 0]
    rows[2] = [R.SKIP, 2, 2, 0xFFFFFF, 0, 0, 15, 15, 0, 0, 0, 0]
    out = R.paint(np.zeros((16, 16, 3), np.uint8), rows)
    assert tuple(out[1, 1]) == (255, 0, 0) and tuple(out[1, 5]) == (0, 255, 0) and tuple(out[2, 5]) == (0, 255, 0)
    assert tuple(out[2, 6]) == (255, 0, 0) and tuple(out[15, 15]) == (0, 0, 0)


def test_plan_order_limiter_and_colours():
    """db.py:283-303 / waymo_imdb.py:208-227 on a hand-made record: reverse row order without a key, the limiter carried
    from class to class (and reset to 15 by the image rule only), uc_gradient going negative and being clamped."""
    k, max_out = 4, 20
    dets = np.zeros((k, max_out, 5), np.float32)
    dets[:, :, 0:4] = [1, 2, 30, 40]
    dets[:, :, 4] = 0.5
    counts = np.array([0, 3, 20, 2], np.int32)
    rows = R.plan(dets, counts, (64, 96), lidar=False)
    assert rows.shape == (60, R.ROW_INTS) and list(rows[:25, 0]) == [R.RECT] * 25 and not rows[25:, 0].any()
    assert list(rows[:, 2]) == list(range(60))
    blue = (rows[:25, 3] >> 16) & 255
    assert list(blue[:3]) == [255, 170, 85]                              # limiter 3
    assert blue[3] == 255 and blue[3 + 15] == 0 and blue[3 + 19] == 0    # limiter back to 15: (15 - 19) / 15 < 0 -> 0
    assert list(blue[23:25]) == [255, 127]                               # limiter 2
    assert ((rows[:25, 3] >> 8) & 255 == 127).all() and (rows[:25, 3] & 255 == 0).all()
    lid = np.zeros((k, max_out, 8), np.float32)
    lid[:, :, 0:7] = [20, 20, 1, 8, 4, 2, 0.3]
    lid[:, :, 7] = 1.0
    rows = R.plan(lid, counts, (64, 96), lidar=True)
    blue = (rows[:25, 3] >> 16) & 255
    assert list(blue[:3]) == [255, 170, 85] and blue[3] == 255 and blue[4] == 170 and blue[6] == 0   # limiter stays 3
    # ties go to the lower row, NaN keys last
    key = np.zeros((2, 4, 6), np.float32)
    key[1, :, 5] = [1.0, 3.0, 3.0, np.nan]
    assert R.class_order(key[1], (5, 1)) == [1, 2, 0, 3]


def _read_png(path):
    """A 20-line reader for what write_png writes: 8-bit RGB, no interlace, filter 0 on every scanline."""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, size = 8, b'', None
    while pos < len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b'IHDR':
            w, h, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', body)
            assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
            size = (h, w)
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(size[0], 1 + size[1] * 3)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(size[0], size[1], 3)


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (64, 96)])
def test_write_png_round_trip(tmp_path, shape):
    from faster_rcnn_pytorch_multimodal_amd.model.draw import write_png
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    path = write_png(str(tmp_path / "a.png"), img)
    np.testing.assert_array_equal(_read_png(path), img)
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "b.png"), img.astype(np.float32))


def test_write_png_is_read_by_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from faster_rcnn_pytorch_multimodal_amd.model.draw import write_png
    img = np.random.default_rng(1).integers(0, 256, (33, 65, 3), dtype=np.uint8)
    path = write_png(str(tmp_path / "a.png"), img[:, ::2][:, :, ::-1])     # a non-contiguous view
    with Image.open(path) as im:
        assert im.mode == 'RGB'
        np.testing.assert_array_equal(np.array(im), img[:, ::2][:, :, ::-1])


class _Inner:
    """The members of lib/datasets/db.py that test_net's drawing reads."""
    name = "synthetic_db"
    num_classes = 2
    _uncertainty_sort_type = 'a_bbox_var'

    def __init__(self, files):
        self._val_index, self._test_index = list(files), []
        self.val_roidb = [{'filename': '/data/val/' + f, 'boxes': np.full((2, 4), i, np.float32),
                           'gt_classes': np.array([1, 0], np.int32)} for i, f in enumerate(files[:2])]

    def path_at(self, i, mode='train'):
        return '/data/val/' + self._val_index[i]

    def find_gt_for_frame(self, filename, mode):            # db.py:182-190
        for roi in self.val_roidb:
            if roi['filename'] == filename:
                return roi
        return None


def test_gt_at_through_reference_db():
    from faster_rcnn_pytorch_multimodal_amd.model.test import ReferenceDb
    db = ReferenceDb(_Inner(['a.npy', 'b.npy', 'c.npy']))
    assert db.gt_at(1, 'val')['boxes'][0, 0] == 1 and list(db.gt_at(0, 'val')['gt_classes']) == [1, 0]
    assert db.gt_at(2, 'val') is None                                     # a frame without ground truth
    assert db.file_at(1, 'val') == '/data/val/b.npy' and db._uncertainty_sort_type == 'a_bbox_var'

    class Bare:
        num_classes, name, _val_index, _test_index = 2, 'bare', ['a'], []

        def path_at(self, i, mode='train'):
            return 'a'
    assert ReferenceDb(Bare()).gt_at(0, 'val') is None and ReferenceDb(Bare())._uncertainty_sort_type is None


def test_file_names_and_folders(tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import draw
    assert draw.frame_file_name('/data/val/images/0001234.png', lidar=False) == 'img-0001234.png'
    assert draw.frame_file_name('/data/val/images/frame_07.npy', lidar=False) == 'img-frame_07.png'
    assert draw.frame_file_name('/data/val/point_clouds/000042.npy', lidar=True) == 'iter_0_000042.png'
    assert draw.frame_file_name('000042', lidar=True) == 'iter_0_000042.png'
    C.reset_cfg()
    try:
        C.cfg.ROOT_DIR = str(tmp_path)
        db = _Inner(['a.npy'])
        folder = draw.draw_folder(db, 'test')
        assert folder == os.path.join(C.get_output_dir(db, mode='test'), 'test_drawn')
        assert not os.path.exists(folder)                                 # naming a folder does not make it
        assert draw.reset_draw_folder(db, 'test') == folder and os.listdir(folder) == []
        open(os.path.join(folder, 'stale.png'), 'wb').close()
        draw.reset_draw_folder(db, 'test')
        assert os.listdir(folder) == []                                   # emptied at the start of a run
    finally:
        C.reset_cfg()


def test_sort_key_columns_follow_the_record_layout():
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model.draw import sort_key_columns
    from faster_rcnn_pytorch_multimodal_amd.nets.uncertainty import num_uncertainty_pos
    C.reset_cfg()
    try:
        assert sort_key_columns('a_bbox_var', 2, False) is None           # flag off: the reference falls back to the row order
        for flag in ("EN_BBOX_ALEATORIC", "EN_CLS_ALEATORIC", "EN_BBOX_EPISTEMIC", "EN_CLS_EPISTEMIC"):
            C.cfg.UC[flag] = True
        # [box 4, score, a_entropy, a_mutual_info, a_cls_var x2, e_entropy, e_mutual_info, e_cls_var x2, a_bbox_var x4, e_bbox_var x4]
        assert sort_key_columns('a_entropy', 2, False) == (5, 1) and sort_key_columns('a_cls_var', 2, False) == (7, 2)
        assert sort_key_columns('e_mutual_info', 2, False) == (10, 1)
        assert sort_key_columns('a_bbox_var', 2, False) == (13, 4) and sort_key_columns('e_bbox_var', 2, False) == (17, 4)
        assert 17 + 4 == 5 + num_uncertainty_pos(2, 4)
        assert sort_key_columns('e_bbox_var', 3, True) == (8 + 5 + 5 + 7, 7)
        assert sort_key_columns('e_cls_var', 2, False) is None and sort_key_columns(None, 2, False) is None
        C.cfg.UC.EN_CLS_ALEATORIC = False
        assert sort_key_columns('e_entropy', 2, False) == (5, 1) and sort_key_columns('a_entropy', 2, False) is None
    finally:
        C.reset_cfg()
