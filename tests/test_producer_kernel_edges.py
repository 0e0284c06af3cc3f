"""The three device data producers at their edges: ``csrc/image_augment.hip`` (image_stencil_kernel<GAUSS | AVERAGE | MEDIAN |
SHARPEN>, image_point_kernel<COPY | NOISE | HUE_SAT | AFFINE | DROPOUT>), ``csrc/image_spatter.hip`` (image_spatter_kernel) and
``csrc/lidar_augment.hip`` (frcnn_lidar_augment_kernel<VEC4, Cam>, also behind ``ops.lidar_fov_filter``), against the numpy
restatements of tests/test_image_augment.py, test_image_spatter.py, test_lidar_augment.py and test_lidar_fov.py, which stay
the arbiters and are imported, not copied.

Method for the uint8 frame kernels.  ``img``, ``out`` and (more than one stage) ``scratch`` are each a ``ByteGuarded`` view;
``scratch`` has exactly ``frcnn_image_augment_ws_bytes(h, w)`` bytes and is filled with POISON_BYTE.  Every case runs at view
offset 0 and at one odd offset (1, 2 or 3 bytes off the dword, all three buffers), and with two output pre-fills, 0xC3 and
0x3C: a byte that was never written cannot carry the reference's value under both.  After every call: all bands intact, the
input unchanged, the result equal to the reference.  The float rows of the LiDAR pass sit between NaN bands (``guarded``)
and the output is pre-filled with a finite sentinel.

Which case reaches which path:

    path                                                         reached by
    image_point_kernel: words (3 dwords per 4 pixels)            view offset 0, h * w >= 4
    image_point_kernel: bytes (words == false)                   view offset 1 / 2 / 3
    image_point_kernel: last partial quad (full == false)        every h * w that is no multiple of 4: (1,1) (1,2) (2,1) (3,3) ...
    image_point_kernel: dword read skipped under flip            flip_* cases at offset 0
    image_point_kernel: second grid-stride trip                  2049 x 4096 (more than 8192 x 256 quads)
    image_stencil_kernel: dword store                            offset 0 and (row * w * 3 + b) % 4 == 0; (17,129), (15,63): changes per row
    image_stencil_kernel: byte store (dst & 3, row tail)         odd offset; every w with w * 3 % 4 != 0
    image_stencil_kernel: partial last tile in x / y             (15,63) (17,129) (2,67) (67,2) (4,65) (65,4)
    reflect101 with halo >= n (several folds)                    gauss5 on n = 2, gauss7 on n = 2..3, gauss9 on n = 2..4, n = 1 everywhere
    ping-pong out -> scratch -> out                              chain gauss9 -> median -> dropout on (3,5) and (17,129)
    argument check: grid y of a stencil stage                    1048561 x 1 (rejected); the same frame with a point stage runs
    image_spatter_kernel: halo (10) wider than the frame         (1,1) (1,70) (70,1) (2,2) (5,6)
    image_spatter_kernel: word == false                          view offset 3; row tails of every w with w * 3 % 4 != 0
    image_spatter_kernel: one tile / one past / two by two       (31,63) (32,64) / (33,65) / (64,128)
    lidar kernel VEC4                                            F = 4, both views 16-byte aligned ("f4_vec", "f4_vec_inplace")
    lidar kernel scalar, stride 4                                F = 4, views moved by one float ("f4_shifted")
    lidar kernel scalar, copy of columns 4..                     F = 5, F = 8 out of place ("f5", "f8"); skipped in place ("f8_inplace")
    lidar kernel: 1 / 2 / 3 workgroups, grid-stride              N = 1 .. 256 / 257 / 513, max_blocks 0, 1, 2
    lidar kernel<Cam = FovParams>                                ops.lidar_fov_filter with a KITTI and a CADC matrix

No tolerance below was taken from the kernels under test.  The bit-exact cases use none.  The banded cases use the constants
of the four modules (T_NOISE, T_HUE_SAT, T_FIELD, T_MASK, T_DECISION, T_BYTE, the LiDAR bounds ulp + sigma * 2e-5, rtol 1e-5
and the 1e-3 band of the rain power ratio, the FOV band), and the CPU tests of this file assert from the float64 restatements
alone that every banded case is well posed (profiles/producer_kernel_edge_tests.md).
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

import guarded_buffers as GB
import test_image_augment as TIA
import test_image_spatter as TIS
import test_lidar_augment as TLA
import test_lidar_fov as TLF
from faster_rcnn_pytorch_multimodal_amd import _hip, ops
from faster_rcnn_pytorch_multimodal_amd.model import config as C
from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import image_augment as IA
from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.image_augment import ImageAugment, Spatter, gaussian_taps
from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.lidar_augment import LidarAugment
from oracle import frcnn_oracle as O

DEV = GB.DEV
FILLS = (0xC3, 0x3C)


@pytest.fixture(autouse=True)
def _fresh_cfg():
    C.reset_cfg()
    IA.set_augmentation_rng(None)
    yield
    IA.set_augmentation_rng(None)
    C.reset_cfg()


# ---------------------------------------------------------------------------------------------------------------
# image_augment: cases
# ---------------------------------------------------------------------------------------------------------------
class RawAffine:
    """An affine record given by its forward 3x3 matrix (the fields ``ops.image_augment_stages`` and ``TIA._affine`` read)."""

    def __init__(self, forward, order, cval):
        self.forward, self.order, self.cval = np.asarray(forward, np.float64), order, cval

    def matrix(self, width, height):
        return self.forward


IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
FAR = [[1.0, 0.0, 1.0e6], [0.0, 1.0, -1.0e6], [0.0, 0.0, 1.0]]      # every source coordinate a million pixels outside
# forward x' = 2 x - 1: the inverse is xs = 0.5 x + 0.5, exactly k + 0.5 at every even x (and y): rintf's half-to-even in the
# nearest warp, fractions of exactly 0.5 in the bilinear one (values on multiples of 1/4: ties in the last rounding too)
HALF = [[2.0, 0.0, -1.0], [0.0, 2.0, -1.0], [0.0, 0.0, 1.0]]

DEGENERATE = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (4, 4), (1, 40), (40, 1), (2, 67), (67, 2), (4, 65), (65, 4), (15, 63),
              (17, 129)]
CHAIN_SHAPES = [(3, 5), (17, 129)]
CHAIN = ImageAugment(stages=(('gaussian', 2.5), ('median', 3)), dropout=(0.3, True), seed=61)

STAGES = {
    "flip": ImageAugment(flip=True),
    "average2": ImageAugment(stages=(('average', 2),)),
    "average3": ImageAugment(stages=(('average', 3),)),
    "median": ImageAugment(stages=(('median', 3),)),
    "sharpen": ImageAugment(stages=(('sharpen', 0.8, 1.3),)),
    "gauss5": ImageAugment(stages=(('gaussian', 1.0),)),
    "gauss7": ImageAugment(stages=(('gaussian', 2.0),)),
    "gauss9": ImageAugment(stages=(('gaussian', 2.5),)),
    "dropout_shared_p0": ImageAugment(dropout=(0.0, False), seed=41),
    "dropout_shared_p1": ImageAugment(dropout=(1.0, False), seed=42),
    "dropout_shared_p05": ImageAugment(dropout=(0.5, False), seed=43),
    "dropout_channel_p0": ImageAugment(dropout=(0.0, True), seed=44),
    "dropout_channel_p1": ImageAugment(dropout=(1.0, True), seed=45),
    "dropout_channel_p05": ImageAugment(dropout=(0.5, True), seed=46),
    "noise_scale0": ImageAugment(stages=(('noise', 0.0),), seed=47),
    "affine_nearest_identity": ImageAugment(affine=RawAffine(IDENTITY, 0, 9)),
    "affine_bilinear_identity": ImageAugment(affine=RawAffine(IDENTITY, 1, 9)),
    "affine_nearest_outside": ImageAugment(affine=RawAffine(FAR, 0, 201)),
    "affine_bilinear_outside": ImageAugment(affine=RawAffine(FAR, 1, 201)),
    "affine_nearest_half": ImageAugment(affine=RawAffine(HALF, 0, 77)),
    "affine_bilinear_half": ImageAugment(affine=RawAffine(HALF, 1, 77)),
    "flip_gauss9": ImageAugment(flip=True, stages=(('gaussian', 2.5),)),
    "flip_dropout_channel_p05": ImageAugment(flip=True, dropout=(0.5, True), seed=48),
    "flip_affine_nearest_half": ImageAugment(flip=True, affine=RawAffine(HALF, 0, 77)),
    "flip_affine_bilinear_half": ImageAugment(flip=True, affine=RawAffine(HALF, 1, 77)),
}
GAUSS_HALO = {"gauss5": 2, "gauss7": 3, "gauss9": 4, "flip_gauss9": 4}

BIG = (2049, 4096)                                                  # 8 392 704 pixels > 8192 blocks x 256 quads x 4
TALL = (16 * 65535 + 1, 1)                                          # one frame row past grid y = 65535 of the stencil tile

# band stages at new sizes: (shape, frame seed) and the (parameter, draw seed) lists of test_image_augment.py
BAND_FRAMES = [((33, 67), 1), ((15, 63), 1)]                        # _frame(shape, seed, colour=False)
BAND_OFFSET = 1


def _odd_offset(shape):
    return 1 + (shape[0] + shape[1]) % 3


@functools.lru_cache(maxsize=None)
def _frame(shape, seed=5, colour=True):
    """A frame of any size >= 1 x 1: noise with saturated and constant pixels (never modified: shared by the cases).
    colour=False leaves the saturated colour out: under a hue shift its middle channel is a tie (k + 0.5) by the integer
    inputs alone (test_image_augment.py's docstring), which on a small frame is more than 1 % of the samples."""
    rng = np.random.default_rng(seed + 1000 * shape[0] + shape[1])
    im = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    flat = im.reshape(-1, 3)
    n = flat.shape[0]
    flat[rng.integers(0, n, max(n // 7, 1))] = 255
    flat[rng.integers(0, n, max(n // 7, 1))] = 0
    if colour:
        flat[rng.integers(0, n, max(n // 9, 1))] = (255, 0, 128)
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def _want(shape, case):
    """The restatement's bytes of a case: computed once, shared, never modified."""
    aug = CHAIN if case == "chain" else STAGES[case]
    out = TIA._restate(np.array(_frame(shape)), aug)
    out.setflags(write=False)
    return out


def _fold(i, n):
    """reflect-101 index for any i, n >= 1, written independently of numpy and of the kernel: walk and bounce."""
    if n == 1:
        return 0
    pos, step = 0, 1
    for _ in range(abs(i)):
        if pos + step < 0 or pos + step >= n:
            step = -step
        pos += step
    return pos                                                       # even about 0: index -k reads what index k reads


def _fold_once_then_clamp(i, n):
    """What the kernel did before this test existed: one fold, then a clamp."""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * n - 2 - i
    return min(max(i, 0), n - 1)


# ---------------------------------------------------------------------------------------------------------------
# CPU: the restatements at these sizes, well-posedness of every banded case, seeds fixed
# ---------------------------------------------------------------------------------------------------------------
def test_restatement_border_is_reflect101_for_every_dimension():
    """np.pad(mode='reflect'), which _gauss / _average / _sharpen of test_image_augment.py restate, against a reflect-101
    index written out by hand, n = 1 .. 12 under every halo the kernels use; and where fold-once-then-clamp departs from it:
    exactly the (n, halo) pairs with 2 <= n <= halo."""
    wrong = set()
    for n in range(1, 13):
        for r in (1, 2, 3, 4):
            got = np.pad(np.arange(n), (r, r), mode='reflect')
            want = [_fold(i, n) for i in range(-r, n + r)]
            assert got.tolist() == want, (n, r)
            if [_fold_once_then_clamp(i, n) for i in range(-r, n + r)] != want:
                wrong.add((n, r))
    assert wrong == {(2, 2), (2, 3), (3, 3), (2, 4), (3, 4), (4, 4)}
    assert np.pad(np.arange(2), (4, 4), mode='reflect').tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    # n == 1: every tap reads the only sample, in both directions, so a normalised blur returns the frame
    for r in (1, 2, 3, 4):
        assert not np.pad(np.arange(1), (r, r), mode='reflect').any()
    one = np.arange(256, dtype=np.uint8).reshape(256, 1, 1, 1).repeat(3, 3)          # every value as a 1 x 1 frame
    for px in one:
        for sigma in (1.0, 2.0, 2.5):
            np.testing.assert_array_equal(TIA._gauss(px, gaussian_taps(sigma)), px)
        for got in (TIA._average(px, 2), TIA._average(px, 3), TIA._median(px), TIA._sharpen(px, 0.0, 1.0)):
            np.testing.assert_array_equal(got, px)
    # a 1 x W frame transposed is a W x 1 frame: the two passes see the same samples (the order of the passes differs,
    # so the comparison is on the value before the final rounding's neighbourhood: at most one count apart)
    row = np.array(_frame((1, 40)))
    for sigma in (1.0, 2.0, 2.5):
        a = TIA._gauss(row, gaussian_taps(sigma)).astype(np.int64)
        b = TIA._gauss(row.transpose(1, 0, 2).copy(), gaussian_taps(sigma)).transpose(1, 0, 2).astype(np.int64)
        assert np.abs(a - b).max() <= 1


def test_image_cases_are_what_their_names_say():
    for shape in DEGENERATE + CHAIN_SHAPES:
        im = np.array(_frame(shape))
        assert im.shape == shape + (3,) and (im == 255).any() and (im == 0).any()
        h, w = shape
        for case, aug in STAGES.items():
            assert len(ops.image_augment_stages(aug, h, w)[1]) <= 1, case
        np.testing.assert_array_equal(_want(shape, "noise_scale0"), im)                       # the identity, exact
        np.testing.assert_array_equal(_want(shape, "dropout_shared_p0"), im)
        np.testing.assert_array_equal(_want(shape, "dropout_channel_p0"), im)
        assert not _want(shape, "dropout_shared_p1").any() and not _want(shape, "dropout_channel_p1").any()
        np.testing.assert_array_equal(_want(shape, "affine_nearest_identity"), im)
        np.testing.assert_array_equal(_want(shape, "affine_bilinear_identity"), im)
        assert (_want(shape, "affine_nearest_outside") == 201).all() and (_want(shape, "affine_bilinear_outside") == 201).all()
        np.testing.assert_array_equal(_want(shape, "flip"), im[:, ::-1])
    assert len(ops.image_augment_stages(CHAIN, 3, 5)[1]) == 3                               # out -> scratch -> out
    # the x.5 warp: the inverse the device receives is exactly 0.5 x + 0.5, so every even coordinate is a tie
    inv = np.linalg.inv(np.asarray(HALF)).astype(np.float32)
    np.testing.assert_array_equal(inv, np.array([[0.5, 0, 0.5], [0, 0.5, 0.5], [0, 0, 1]], np.float32))
    im = np.array(_frame((4, 4)))
    near = _want((4, 4), "affine_nearest_half")
    # xs = 0.5, 1, 1.5, 2 -> rint = 0, 1, 2, 2 (half to even, not half up: 0.5 -> 0)
    np.testing.assert_array_equal(near, im[np.ix_([0, 1, 2, 2], [0, 1, 2, 2])])
    assert not np.array_equal(near, im[np.ix_([1, 1, 2, 2], [1, 1, 2, 2])])
    # dropout at 0.5 drops something and keeps something on the frames that have room for it
    for shape in ((17, 129), (15, 63), (65, 4)):
        for case in ("dropout_shared_p05", "dropout_channel_p05"):
            kept = (_want(shape, case) == np.array(_frame(shape)))
            assert 0.3 < kept.mean() < 0.8, (shape, case)
    # the second grid-stride trip exists
    assert (BIG[0] * BIG[1] + 3) // 4 > 8192 * 256 and BIG[0] * BIG[1] <= 1 << 29
    assert (TALL[0] + 15) // 16 == 65536 and TALL[0] * TALL[1] <= 1 << 29


def test_band_cases_are_well_posed():
    """The condition of the band comparisons ("share of samples inside the band < 1 %"), from the float64 restatement alone,
    for every added (shape, case)."""
    for shape, fseed in BAND_FRAMES:
        frame = np.array(_frame(shape, fseed, False))
        for scale, seed in TIA.NOISE_CASES:
            share = TIA._band_share(TIA._noise_pre(frame, scale, seed), TIA.T_NOISE)
            print("noise %s scale %g seed %d: share in band %.3g" % (shape, scale, seed, share))
            assert share < 0.01, (shape, scale, seed, share)
        for hue, sat in TIA.HUE_SAT_CASES:
            share = TIA._band_share(TIA._hue_sat_pre(frame, hue, sat), TIA.T_HUE_SAT)
            print("hue_sat %s (%d, %d): share in band %.3g" % (shape, hue, sat, share))
            assert share < 0.01, (shape, hue, sat, share)
    # the seed_dev case of the noise stage
    share = TIA._band_share(TIA._noise_pre(np.array(_frame((17, 129))), 8.0, 1), TIA.T_NOISE)
    assert share < 0.01


def test_tall_frame_with_a_stencil_stage_is_rejected_without_a_gpu():
    """h = 16 * 65535 + 1 needs grid y = 65536: an argument error with a message, nothing launched (the addresses are fake)."""
    import ctypes
    lib = _hip.load()
    h, w = TALL
    img, out, scr = 1 << 24, 2 << 24, 3 << 24
    need = lib.frcnn_image_augment_ws_bytes(h, w)

    def call(stages, h=h):
        flat = []
        for _, vals in stages:
            flat += list(vals) + [0.0] * (ops.IMG_NUM_PARAMS - len(vals))
        codes = (ctypes.c_int * len(stages))(*[s[0] for s in stages])
        return lib.frcnn_image_augment(img, h, w, 0, len(stages), codes, _hip.float_array(flat), 1, None, scr, need, out, None,
                                       None)

    gauss = (ops.IMG_GAUSS, [5.0] + [float(t) for t in gaussian_taps(1.0)])
    for stage in ((ops.IMG_MEDIAN, []), (ops.IMG_AVERAGE, [3.0]), (ops.IMG_SHARPEN, [2.0, -0.1]), gauss):
        assert call((stage,)) == -1, stage
        msg = lib.frcnn_last_error()
        assert b"frame size" in msg and b"stencil" in msg and str(h).encode() in msg, msg
    # the stencil stage need not be the first one
    assert call(((ops.IMG_DROPOUT, [0.1, 0.0]), (ops.IMG_MEDIAN, []))) == -1 and b"stage 1" in lib.frcnn_last_error()


# ---------------------------------------------------------------------------------------------------------------
# GPU: image_augment
# ---------------------------------------------------------------------------------------------------------------
def _augment_guarded(hip, im, aug, offset, fill, seed_dev=None, debug_pre=None, expect_error=None):
    """One call with img / out / scratch as guarded views ``offset`` bytes off the allocation's alignment.  Asserts the bands
    and the input; returns the output bytes."""
    h, w = im.shape[:2]
    n = h * w * 3
    src = GB.ByteGuarded(n, 0, offset)
    src.view.copy_(torch.from_numpy(np.ascontiguousarray(im)).reshape(-1))
    dst = GB.ByteGuarded(n, fill, offset)
    scratch = None
    if len(ops.image_augment_stages(aug, h, w)[1]) > 1:
        scratch = GB.ByteGuarded(hip.frcnn_image_augment_ws_bytes(h, w), GB.POISON_BYTE, offset)
    kw = dict(out=dst.view.view(h, w, 3), scratch=None if scratch is None else scratch.view, seed_dev=seed_dev, debug_pre=debug_pre)
    if expect_error is None:
        assert ops.image_augment(src.view.view(h, w, 3), aug, **kw) is kw["out"]
    else:
        with pytest.raises(_hip.HipError, match=expect_error):
            ops.image_augment(src.view.view(h, w, 3), aug, **kw)
    torch.cuda.synchronize()
    assert src.intact() and dst.intact() and (scratch is None or scratch.intact()), "a guard band was written"
    assert torch.equal(src.view.cpu(), torch.from_numpy(np.ascontiguousarray(im)).reshape(-1)), "the input was written"
    return dst.view.cpu().numpy().reshape(h, w, 3)


def _exact_case(hip, shape, case, failures):
    aug = CHAIN if case == "chain" else STAGES[case]
    im, want = np.array(_frame(shape)), _want(shape, case)
    for offset in (0, _odd_offset(shape)):
        for fill in FILLS:
            got = _augment_guarded(hip, im, aug, offset, fill)
            bad = np.argwhere(got != want)
            if len(bad):
                failures.append("%dx%d-%s offset %d fill 0x%02X: %d samples differ, first at %s: got %d want %d" % (
                    shape + (case, offset, fill, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DEGENERATE, ids=lambda s: "%dx%d" % s)
def test_image_stages_are_bit_equal_on_degenerate_frames(hip, shape):
    failures = []
    for case in STAGES:
        _exact_case(hip, shape, case, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_three_stage_chain_ping_pongs_through_scratch(hip, shape):
    failures = []
    _exact_case(hip, shape, "chain", failures)
    assert not failures, "\n".join(failures)


def _dropout_mask(n, p, seed):
    return O.uniform01(seed, TIA.STREAM['image_dropout'], np.arange(n)) < np.float32(p)


@pytest.mark.gpu
def test_point_kernel_second_grid_stride_trip(hip):
    """2049 x 4096: 2 098 176 quads on a grid capped at 8192 x 256 threads, so 1024 threads come round a second time.
    Compared on the device (the frame is 25 MB); noise at scale 0 is the identity (asserted of the restatement on the CPU)."""
    h, w = BIG
    im = np.random.default_rng(7).integers(0, 256, (h, w, 3), dtype=np.uint8)
    drop = _dropout_mask(h * w, 0.3, 71).reshape(h, w, 1)
    wants = {"flip": (ImageAugment(flip=True), np.ascontiguousarray(im[:, ::-1])),
             "dropout_shared": (ImageAugment(dropout=(0.3, False), seed=71), np.where(drop, 0, im).astype(np.uint8)),
             "noise_scale0": (ImageAugment(stages=(('noise', 0.0),), seed=72), im)}
    assert 0.29 < drop.mean() < 0.31
    n = h * w * 3
    src = GB.ByteGuarded(n, 0, 0)
    host = torch.from_numpy(im).reshape(-1)
    src.view.copy_(host)
    for name, (aug, want) in wants.items():
        want_dev = torch.from_numpy(want).to(DEV)
        for fill in FILLS:
            dst = GB.ByteGuarded(n, fill, 0)
            ops.image_augment(src.view.view(h, w, 3), aug, out=dst.view.view(h, w, 3))
            torch.cuda.synchronize()
            assert src.intact() and dst.intact(), name
            differ = dst.view.view(h, w, 3) != want_dev
            assert not bool(differ.any()), "%s fill 0x%02X: %d samples differ, first at flat index %d" % (
                name, fill, int(differ.sum()), int(differ.reshape(-1).nonzero()[0]))
    assert torch.equal(src.view.cpu(), host)


@pytest.mark.gpu
def test_band_stages_at_new_sizes(hip):
    """Noise > 0 and hue / saturation on (33,67) and (15,63), byte paths (view offset 1): the method and the constants of
    test_image_augment.py; the value before rounding lands in a NaN-guarded float view."""
    worst = {"noise": 0.0, "hue_sat": 0.0}
    for shape, fseed in BAND_FRAMES:
        frame = np.array(_frame(shape, fseed, False))
        cases = [("noise", ImageAugment(stages=(('noise', scale),), seed=seed), TIA._noise_pre(frame, scale, seed), TIA.T_NOISE)
                 for scale, seed in TIA.NOISE_CASES]
        cases += [("hue_sat", ImageAugment(stages=(('hue_sat', hue, sat),)), TIA._hue_sat_pre(frame, hue, sat), TIA.T_HUE_SAT)
                  for hue, sat in TIA.HUE_SAT_CASES]
        for kind, aug, v, t in cases:
            what = "%s %s %s" % (kind, shape, aug.stages[0][1:])
            results = []
            for fill in FILLS:
                buf, pre = GB.guarded(v.size)
                got = _augment_guarded(hip, frame, aug, BAND_OFFSET, fill, debug_pre=pre)
                assert GB.guards_intact(buf, v.size), what
                pre = pre.cpu().numpy().astype(np.float64).reshape(v.shape)
                assert np.isfinite(pre).all(), what                                  # every sample's value was written
                err = float(np.abs(pre - v).max())
                worst[kind] = max(worst[kind], err)
                print("%s fill 0x%02X: max |device - float64| before rounding %.3g (T = %.3g), share in band %.3g"
                      % (what, fill, err, t, TIA._band_share(v, t)))
                TIA._check_band(got, v, t, what)
                assert err <= t, what
                np.testing.assert_array_equal(got, _augment_guarded(hip, frame, aug, BAND_OFFSET, fill))   # without debug_pre
                results.append(got)
            np.testing.assert_array_equal(results[0], results[1])
    print("largest gap: noise %.3g of T_NOISE %.3g, hue_sat %.3g of T_HUE_SAT %.3g"
          % (worst["noise"], TIA.T_NOISE, worst["hue_sat"], TIA.T_HUE_SAT))


def _seed_word(value):
    return torch.tensor([value], dtype=torch.int32, device=DEV)


@pytest.mark.gpu
def test_image_augment_seed_word_wraps_like_the_host_sum(hip):
    """seed 0xFFFFFFFF + *seed_dev 2 == seed 1 (uint32 wrap) == the restatement at seed 1: dropout (exact) and noise (band)."""
    shape = (17, 129)
    im = np.array(_frame(shape))
    for offset in (0, _odd_offset(shape)):
        for fill in FILLS:
            for per_channel in (False, True):
                host = ImageAugment(dropout=(0.4, per_channel), seed=1)
                moved = ImageAugment(dropout=(0.4, per_channel), seed=0xFFFFFFFF)
                want = TIA._restate(im, host)
                assert 0.3 < (want != im).mean() < 0.5
                np.testing.assert_array_equal(_augment_guarded(hip, im, host, offset, fill), want)
                np.testing.assert_array_equal(_augment_guarded(hip, im, moved, offset, fill, seed_dev=_seed_word(2)), want)
                assert (_augment_guarded(hip, im, moved, offset, fill) != want).mean() > 0.1      # the word is read
            host = ImageAugment(stages=(('noise', 8.0),), seed=1)
            moved = ImageAugment(stages=(('noise', 8.0),), seed=0xFFFFFFFF)
            a = _augment_guarded(hip, im, host, offset, fill)
            TIA._check_band(a, TIA._noise_pre(im, 8.0, 1), TIA.T_NOISE, "noise seed 1")
            np.testing.assert_array_equal(_augment_guarded(hip, im, moved, offset, fill, seed_dev=_seed_word(2)), a)
            assert (_augment_guarded(hip, im, moved, offset, fill) != a).mean() > 0.5


@pytest.mark.gpu
def test_tall_frame_stencil_rejected_point_stage_runs(hip):
    """1048561 x 1: a stencil stage would need grid y = 65536 and is refused before anything is launched (the output keeps
    its pre-fill); the pointwise stages run on their capped 1-D grid and equal the restatement."""
    h, w = TALL
    im = np.random.default_rng(9).integers(0, 256, (h, w, 3), dtype=np.uint8)
    for fill in FILLS:
        for aug in (ImageAugment(stages=(('median', 3),)), ImageAugment(flip=True, stages=(('gaussian', 2.5),)),
                    ImageAugment(stages=(('noise', 0.0), ('average', 2)), seed=3)):
            got = _augment_guarded(hip, im, aug, 0, fill, expect_error=r"failed \(-1\).*stencil")
            assert (got == fill).all()
        point = ImageAugment(dropout=(0.3, False), seed=81)
        want = TIA._dropout(im, 0.3, False, 81)
        assert 0.29 < (want != im).mean() < 0.31
        for offset in (0, 3):
            np.testing.assert_array_equal(_augment_guarded(hip, im, point, offset, fill), want)
        np.testing.assert_array_equal(_augment_guarded(hip, im, ImageAugment(flip=True), 0, fill), im)     # w == 1: a copy


# ---------------------------------------------------------------------------------------------------------------
# image_spatter
# ---------------------------------------------------------------------------------------------------------------
TINY_PIXELS = 64                  # below this the share conditions of test_image_spatter.py cannot hold statistically
# (shape, severity, seed, mud): seed = the first one whose float64 restatement has NO pixel in either decision band and
# meets ``mud``: True = some pixel is mud, False = none is, None = no condition (tiny) / at least 5 % mud (the others).
# Found on the CPU by ``_first_seed`` and asserted by test_spatter_seeds_are_the_first_well_posed_ones.
SPATTER_CASES = [((1, 1), 5, 1, True), ((1, 1), 5, 0, False), ((1, 70), 5, 0, None), ((70, 1), 5, 0, None), ((2, 2), 5, 0, False),
                 ((2, 2), 5, 1, True), ((5, 6), 5, 0, None), ((31, 63), 5, 0, None), ((32, 64), 5, 0, None), ((33, 65), 5, 0, None),
                 ((64, 128), 5, 1, None)]
SPATTER_SEED_WORD_CASE = ((33, 65), 5)


def _spatter_bands(shape, severity, seed):
    """(pixels in the first decision band, in the second, share of mud) of the float64 restatement under its own decisions."""
    liquid = TIS._liquid64(shape, severity, seed)
    thr = TIS._thr(severity)
    m = TIS._mask64(liquid > thr, severity)
    return (int((np.abs(liquid - thr) <= TIS.T_DECISION).sum()), int((np.abs(m - TIS.CUT) <= TIS.T_DECISION).sum()),
            float((m >= TIS.CUT).mean()))


def _spatter_ok(shape, severity, seed, mud):
    band1, band2, share = _spatter_bands(shape, severity, seed)
    if band1 or band2:
        return False
    if mud is None:
        return shape[0] * shape[1] < TINY_PIXELS or share >= TIS.MIN_MUD_SHARE
    return (share > 0) == mud


def _first_seed(shape, severity, mud):
    for seed in range(1000):
        if _spatter_ok(shape, severity, seed, mud):
            return seed
    raise AssertionError("no seed for %s" % (shape,))


def test_spatter_seeds_are_the_first_well_posed_ones():
    """Every case: no pixel of the float64 restatement in either decision band (so every decision has one admissible answer
    and every byte one value, or two inside the +-1 truncation band), and the seed is the first such."""
    tiny_mud = set()
    for shape, severity, seed, mud in SPATTER_CASES:
        band1, band2, share = _spatter_bands(shape, severity, seed)
        print("%s severity %d seed %d: pixels in the decision bands %d / %d, mud %.1f %%" % (shape, severity, seed, band1, band2,
                                                                                       100 * share))
        assert band1 == 0 and band2 == 0, (shape, seed)
        assert seed == _first_seed(shape, severity, mud), (shape, mud, _first_seed(shape, severity, mud))
        if shape[0] * shape[1] < TINY_PIXELS:
            tiny_mud.add(share > 0)
        else:
            assert share >= TIS.MIN_MUD_SHARE, (shape, share)
        assert TIS._frame(shape, seed).shape == shape + (3,)
    assert tiny_mud == {True, False}
    assert {s for s, _, _, _ in SPATTER_CASES} >= {(1, 1), (1, 70), (70, 1), (2, 2), (5, 6), (31, 63), (32, 64), (33, 65), (64, 128)}


def _spatter_guarded(im, rec, offset, fill, seed_dev=None):
    h, w = im.shape[:2]
    n = h * w * 3
    src = GB.ByteGuarded(n, 0, offset)
    src.view.copy_(torch.from_numpy(im).reshape(-1))
    dst = GB.ByteGuarded(n, fill, offset)
    lbuf, liquid = GB.guarded(h * w)
    mbuf, mask = GB.guarded(h * w)
    out = ops.image_spatter(src.view.view(h, w, 3), rec, out=dst.view.view(h, w, 3), seed_dev=seed_dev, debug_liquid=liquid,
                            debug_mask=mask)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.ptr
    assert src.intact() and dst.intact() and GB.guards_intact(lbuf, h * w) and GB.guards_intact(mbuf, h * w), "a guard band was written"
    assert torch.equal(src.view.cpu(), torch.from_numpy(im).reshape(-1)), "the input was written"
    got = dst.view.cpu().numpy().reshape(h, w, 3)
    plain = GB.ByteGuarded(n, fill, offset)                                           # the debug outputs change nothing
    ops.image_spatter(src.view.view(h, w, 3), rec, out=plain.view.view(h, w, 3), seed_dev=seed_dev)
    torch.cuda.synchronize()
    assert plain.intact() and np.array_equal(plain.view.cpu().numpy().reshape(h, w, 3), got)
    return got, liquid.cpu().numpy().reshape(h, w), mask.cpu().numpy().reshape(h, w)


def _check_spatter(shape, severity, seed, offset, fill, run_seed=None, seed_dev=None):
    """Steps 1-5 of test_image_spatter.py::_check_against_restatement with the decisions pinned by the restatement itself
    (no pixel is in a decision band), in guarded buffers."""
    what = "%s severity %d seed %d offset %d fill 0x%02X" % (shape, severity, seed, offset, fill)
    im = TIS._frame(shape, seed)
    got, liquid_dev, mask_dev = _spatter_guarded(im, Spatter(severity, seed if run_seed is None else run_seed), offset, fill, seed_dev)
    assert np.isfinite(liquid_dev).all() and np.isfinite(mask_dev).all(), what      # every in-frame position was written
    liquid = TIS._liquid64(shape, severity, seed)
    thr = TIS._thr(severity)
    err1 = float(np.abs(liquid_dev.astype(np.float64) - liquid).max())
    assert err1 <= TIS.T_FIELD, (what, err1)
    decision = liquid > thr
    assert np.array_equal(liquid_dev > np.float32(thr), decision), what
    m = TIS._mask64(decision, severity)
    err3 = float(np.abs(mask_dev.astype(np.float64) - m).max())
    assert err3 <= TIS.T_MASK, (what, err3)
    mud = m >= TIS.CUT
    assert np.array_equal(mask_dev >= np.float32(TIS.CUT), mud), what
    v = TIS._blend64(im, np.where(mud, m, 0.0))
    diff = got.astype(np.int64) - np.floor(v).astype(np.int64)
    clear = np.abs(v - np.rint(v)) > TIS.T_BYTE
    assert (diff[clear] == 0).all(), "%s: %d bytes differ outside the band" % (what, int((diff[clear] != 0).sum()))
    assert (np.abs(diff) <= 1).all(), what
    assert np.array_equal(got[~mud], im[~mud]), what                                 # m = 0: bit for bit the input
    return got, err1, err3, int(mud.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPATTER_CASES, ids=lambda c: "%dx%d-seed%d-%s" % (c[0] + (c[2], {None: "any", True: "mud", False: "clean"}[c[3]])))
def test_spatter_on_tiny_and_straddling_frames(hip, case):
    shape, severity, seed, mud = case
    results = []
    for offset in (0, 3):
        for fill in FILLS:
            got, err1, err3, count = _check_spatter(shape, severity, seed, offset, fill)
            print("%s offset %d fill 0x%02X: field err %.3g (T %.3g), mask err %.3g (T %.3g), %d mud pixels"
                  % (shape, offset, fill, err1, TIS.T_FIELD, err3, TIS.T_MASK, count))
            results.append(got)
            if mud is not None:
                assert (count > 0) == mud
    for other in results[1:]:
        np.testing.assert_array_equal(other, results[0])                             # offsets and pre-fills agree byte for byte


@pytest.mark.gpu
def test_spatter_seed_word_wraps_like_the_host_sum(hip):
    shape, severity = SPATTER_SEED_WORD_CASE
    assert _spatter_bands(shape, severity, 1)[:2] == (0, 0)
    for offset in (0, 3):
        for fill in FILLS:
            host = _check_spatter(shape, severity, 1, offset, fill)[0]
            moved = _check_spatter(shape, severity, 1, offset, fill, run_seed=0xFFFFFFFF, seed_dev=_seed_word(2))[0]
            np.testing.assert_array_equal(moved, host)
            im = TIS._frame(shape, 1)
            assert not np.array_equal(_spatter_guarded(im, Spatter(severity, 0xFFFFFFFF), offset, fill)[0], host)


# ---------------------------------------------------------------------------------------------------------------
# lidar_augment_points / lidar_fov_filter
# ---------------------------------------------------------------------------------------------------------------
POINT_COUNTS = [1, 63, 64, 65, 255, 256, 257, 513]
SENTINEL = -7777.0
# name -> (F, floats the views are moved off the 16-byte alignment, in place)
LIDAR_PATHS = {"f4_vec": (4, 0, False), "f4_shifted": (4, 1, False), "f5": (5, 0, False), "f8": (8, 0, False),
               "f4_vec_inplace": (4, 0, True), "f8_inplace": (8, 0, True)}
LIDAR_EXACT = dict(TLA.EXACT_CASES, rotate_0=LidarAugment(rotation=0.0), rotate_90=LidarAugment(rotation=math.pi / 2),
                   rotate_90_swap_flip=LidarAugment(rotation=math.pi / 2, swap_xy=True, flip_x=True, flip_y=True))
GAUSS_DROPOUT = LidarAugment(gauss=(0.07, 0.05, 0.03), p_keep=0.83, seed=0xC0FFEE)
TEST_DROPOUT = LidarAugment(test_dropout=True, seed=321)
# the first seed from 1001 on for which no point of any cloud below lies within 1e-3 of the power threshold (CPU test)
RAIN = LidarAugment(rain_rate=10.0, rain_max_range=200.0, seed=1008)
SEED_WORD_MIX = LidarAugment(gauss=(0.07, 0.05, 0.03), p_keep=0.83, rain_rate=10.0, rain_max_range=200.0, seed=1)
LO, HI = np.array(TLA.EXTENTS[:3], np.float32), np.array(TLA.EXTENTS[3:], np.float32)


@functools.lru_cache(maxsize=None)
def _cloud(n, f, kind):
    """(n, f) float32 rows.  mixed: about a quarter outside the extents, and (n >= 12) one point on each of the six range
    faces - the lower ones are inside (>= lo), the upper ones outside (< hi); all_in / all_out; faces: every point on a face."""
    rng = np.random.default_rng(1000 * n + 10 * f + len(kind))
    inside = rng.uniform(LO + 0.01, HI - 0.01, (n, 3))
    rows = rng.uniform(0.0, 3.0, (n, f)).astype(np.float32)
    if kind == "all_in":
        rows[:, :3] = inside
    elif kind == "all_out":
        axis, up = rng.integers(0, 3, n), rng.integers(0, 2, n).astype(bool)
        out = inside.copy()
        out[np.arange(n), axis] = np.where(up, HI[axis] + rng.uniform(0, 2, n), LO[axis] - rng.uniform(0.001, 2, n))
        rows[:, :3] = out
    elif kind == "faces":
        pts = inside.astype(np.float32)
        face = np.arange(n) % 6
        pts[np.arange(n), face % 3] = np.where(face < 3, LO[face % 3], HI[face % 3])
        rows[:, :3] = pts
    else:
        rows[:, :3] = rng.uniform(LO - [2, 2, 0.2], HI + [2, 2, 0.2], (n, 3))
        if n >= 12:
            at = rng.permutation(n)[:6]
            rows[at, :3] = inside[at]
            for j in range(6):
                rows[at[j], j % 3] = LO[j % 3] if j < 3 else HI[j % 3]
        elif n == 1:
            rows[0, :3] = inside[0]
    rows.setflags(write=False)
    return rows


def _lidar_guarded(rows, path, call):
    """Run ``call(points_view, out_view)`` with the rows (and the output, unless in place) between NaN bands; returns
    (output rows on the host, what ``call`` returned)."""
    f, shift, inplace = LIDAR_PATHS[path]
    n = rows.shape[0]
    assert rows.shape[1] == f
    numel = n * f

    def view():
        buf, flat = GB.guarded(numel + shift)
        flat[:shift] = float("nan")
        return buf, flat[shift:].view(n, f)

    ibuf, pts = view()
    pts.copy_(torch.from_numpy(np.array(rows)))
    assert (pts.data_ptr() % 16 == 0) == (shift == 0)
    if inplace:
        obuf, out = ibuf, pts
    else:
        obuf, out = view()
        out.fill_(SENTINEL)
    result = call(pts, out)
    torch.cuda.synchronize()
    for buf in (ibuf, obuf):
        assert GB.guards_intact(buf, numel + shift) and bool(torch.isnan(buf[GB.GUARD:GB.GUARD + shift]).all()), "a guard band was written"
    got = out.cpu().numpy()
    if not inplace:
        assert pts.cpu().numpy().tobytes() == rows.tobytes(), "the input was written"
        assert (got != np.float32(SENTINEL)).all(), "a row was not written"
    return got, result


def _augment(rows, path, aug, max_blocks=0, seed=None, seed_dev=None):
    def call(pts, out):
        res, kept = ops.lidar_augment_points(pts, aug, aug.seed if seed is None else seed, TLA.EXTENTS, out=out,
                                             max_blocks=max_blocks, seed_dev=seed_dev)
        assert res is out
        return kept
    got, kept = _lidar_guarded(rows, path, call)
    return got, int(kept.item())


def _check_exact(rows, path, name, max_blocks):
    what = "%s N=%d %s max_blocks=%d" % (path, rows.shape[0], name, max_blocks)
    aug = LIDAR_EXACT[name]
    pts = np.array(rows)
    want, keep, _ = TLA._restate(pts, aug, np.float32)
    assert want.dtype == np.float32
    got, kept = _augment(rows, path, aug, max_blocks)
    assert np.isnan(got[~keep, :3]).all() and not np.isnan(got[keep, :3]).any(), what
    np.testing.assert_array_equal(got[:, 3:].view(np.uint32), pts[:, 3:].view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32), err_msg=what)
    assert kept == TLA._final_count(want, keep), what
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(LIDAR_PATHS))
def test_lidar_exact_steps_on_small_clouds(hip, path):
    """Pre-filter, flips, swap, rotation by 0 and pi / 2 (c, s rounded once, one rounding per operation): bit-equal to the
    float32 restatement at every point count around the wave and workgroup sizes, under 1, 2 and the default grid."""
    f = LIDAR_PATHS[path][0]
    for n in POINT_COUNTS:
        for name in sorted(LIDAR_EXACT):
            for max_blocks in (0, 1, 2):
                keep = _check_exact(_cloud(n, f, "mixed"), path, name, max_blocks)
        assert n < 12 or 0 < keep.sum() < n
        for name in ("prefilter", "swap_flip_xy"):
            assert _check_exact(_cloud(n, f, "all_in"), path, name, 0).all()
            assert not _check_exact(_cloud(n, f, "all_out"), path, name, 0).any()         # kept == 0, every row NaN
            on_face = _check_exact(_cloud(n, f, "faces"), path, name, 0)
            np.testing.assert_array_equal(on_face, (np.arange(n) % 6) < 3)                 # >= lo stays, < hi: the face itself goes


def _rain_unsure(rows):
    _, _, ex = TLA._restate(np.array(rows), RAIN, np.float64)
    return ex["before_rain"] & (np.abs(ex["ratio"] - 1.0) <= 1e-3)


def test_lidar_rain_cases_are_well_posed():
    """No point of any rain case lies within 1e-3 of the power threshold (float64 restatement): the keep mask is pinned."""
    for f in (4, 5, 8):
        for n in POINT_COUNTS:
            assert not _rain_unsure(_cloud(n, f, "mixed")).any(), (n, f)
    n, f = 513, 4
    for width in (4, 8):
        _, _, ex = TLA._restate(np.array(_cloud(n, width, "mixed")), SEED_WORD_MIX, np.float64)
        assert not (ex["before_rain"] & (np.abs(ex["ratio"] - 1.0) <= 1e-3)).any()
    for kind, count in (("all_in", n), ("all_out", 0)):
        rows = _cloud(n, f, kind)
        assert int(TLA._in_range(rows[:, 0], rows[:, 1], rows[:, 2]).sum()) == count
    faces = _cloud(n, f, "faces")
    np.testing.assert_array_equal(TLA._in_range(faces[:, 0], faces[:, 1], faces[:, 2]), (np.arange(n) % 6) < 3)
    # golden FOV points: every point count finds inside and outside points, none near an edge
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_fov.npz")) as z:
        for name in FOV_CASES:
            db = str(z[name + "_db"])
            uv = z[name + "_uv"]
            want = TLF._flags(uv, TLF.IMG_SIZE[db])
            assert not TLF._near_edge(uv, TLF.IMG_SIZE[db], TLF.BAND[db]).any()
            assert want.sum() >= max(POINT_COUNTS) and (~want).sum() >= max(POINT_COUNTS)


def _draw_bounds(got, want, keep, sigma, what):
    """|err| <= ulp(coordinate) + sigma * 2e-5 per axis (test_lidar_augment.py)."""
    for k in range(3):
        err = np.abs(got[keep, k].astype(np.float64) - want[keep, k])
        s = sigma[k] if np.ndim(sigma[k]) == 0 else sigma[k][keep]
        bound = np.spacing(np.abs(want[keep, k]).astype(np.float32)).astype(np.float64) + s * 2e-5
        assert (err <= bound).all(), (what, k, float((err / bound).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(LIDAR_PATHS))
def test_lidar_draw_steps_on_small_clouds(hip, path):
    """Gauss + dropout, test dropout and rain under the bounds of test_lidar_augment.py; the keep masks are the replayed ones."""
    f = LIDAR_PATHS[path][0]
    for n in POINT_COUNTS:
        rows = _cloud(n, f, "mixed")
        pts = np.array(rows)
        for max_blocks in (0, 1, 2):
            what = "%s N=%d max_blocks=%d" % (path, n, max_blocks)
            # Gaussian distortion + dropout
            want, keep, _ = TLA._restate(pts, GAUSS_DROPOUT, np.float64)
            got, kept = _augment(rows, path, GAUSS_DROPOUT, max_blocks)
            assert np.isnan(got[~keep, :3]).all() and not np.isnan(got[keep, :3]).any(), what
            _draw_bounds(got, want, keep, GAUSS_DROPOUT.gauss, what)
            np.testing.assert_array_equal(got[:, 3:].view(np.uint32), pts[:, 3:].view(np.uint32))
            assert kept == TLA._final_count(got, keep), what
            # test-time dropout: integer arithmetic
            want, keep, _ = TLA._restate(pts, TEST_DROPOUT, np.float32)
            got, kept = _augment(rows, path, TEST_DROPOUT, max_blocks)
            assert np.isnan(got[~keep, :3]).all(), what
            np.testing.assert_array_equal(got[keep].view(np.uint32), pts[keep].view(np.uint32))
            np.testing.assert_array_equal(got[:, 3:].view(np.uint32), pts[:, 3:].view(np.uint32))
            assert kept == int(keep.sum()), what
            # rain
            want, keep, ex = TLA._restate(pts, RAIN, np.float64)
            got, kept = _augment(rows, path, RAIN, max_blocks)
            alive = ~np.isnan(got[:, 0])
            assert np.isnan(got[~alive, :3]).all() and not np.isnan(got[alive, :3]).any(), what
            np.testing.assert_array_equal(alive, keep, err_msg=what)                  # no point is near the threshold (CPU test)
            _draw_bounds(got, want, keep, [ex["sigma"]] * 3, what)
            np.testing.assert_allclose(got[keep, 3].astype(np.float64), want[keep, 3], rtol=1e-5, atol=0, err_msg=what)
            np.testing.assert_array_equal(got[:, 4:].view(np.uint32), pts[:, 4:].view(np.uint32))
            assert kept == TLA._final_count(got, alive), what


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["f4_vec", "f4_shifted", "f8", "f8_inplace"])
def test_lidar_seed_word_wraps_like_the_host_sum(hip, path):
    """gauss + dropout + rain: seed 0xFFFFFFFF + *seed_dev 2 gives the rows of seed 1, bit for bit, and those follow the
    float64 restatement at seed 1."""
    rows = _cloud(513, LIDAR_PATHS[path][0], "mixed")
    pts = np.array(rows)
    host, kept_host = _augment(rows, path, SEED_WORD_MIX, seed=1)
    moved, kept_moved = _augment(rows, path, SEED_WORD_MIX, seed=0xFFFFFFFF, seed_dev=_seed_word(2))
    assert moved.tobytes() == host.tobytes() and kept_moved == kept_host
    plain, _ = _augment(rows, path, SEED_WORD_MIX, seed=0xFFFFFFFF)
    assert not np.array_equal(np.isnan(plain[:, 0]), np.isnan(host[:, 0]))            # the word is read
    want, keep, ex = TLA._restate(pts, SEED_WORD_MIX, np.float64)
    np.testing.assert_array_equal(~np.isnan(host[:, 0]), keep)
    assert 0 < keep.sum() < len(keep) and kept_host == TLA._final_count(host, keep)
    # the rain moves a point by its own draw on top of the distortion: ulp + (gauss sigma + rain sigma) * 2e-5
    _draw_bounds(host, want, keep, [SEED_WORD_MIX.gauss[k] + ex["sigma"] for k in range(3)], path)


FOV_CASES = ["kitti_plain", "cadc_plain"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FOV_CASES)
def test_fov_filter_on_small_clouds(hip, golden_dir, name, tmp_path):
    """ops.lidar_fov_filter at the same point counts, row widths, alignments and grids: the keep mask is the reference's
    flags on the golden points (none of them near an image edge), kept rows are the input rows, rejected rows NaN."""
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import lidar_calib
    with np.load(os.path.join(golden_dir, "lidar_fov.npz")) as z:
        golden = {k: z[k] for k in z.files}
    db, calib, xyz, uv_ref = TLF._case(golden, name, tmp_path)
    m = lidar_calib.load_projection(calib, db)
    size = TLF.IMG_SIZE[db]
    flags = TLF._flags(uv_ref, size)
    inside, outside = np.where(flags)[0], np.where(~flags)[0]
    rng = np.random.default_rng(3)
    for path in sorted(LIDAR_PATHS):
        f = LIDAR_PATHS[path][0]
        for n in POINT_COUNTS:
            picks = {"mixed": rng.permutation(len(flags))[:n], "all_in": inside[rng.permutation(len(inside))[:n]],
                     "all_out": outside[rng.permutation(len(outside))[:n]]}
            for kind, idx in picks.items():
                rows = TLF._rows(xyz[idx], f, seed=n)
                want = flags[idx]
                for max_blocks in ((0, 1, 2) if kind == "mixed" else (0,)):
                    what = "%s %s N=%d %s max_blocks=%d" % (name, path, n, kind, max_blocks)

                    def call(pts, out):
                        res, kept = ops.lidar_fov_filter(pts, m, size, out=out, max_blocks=max_blocks)
                        assert res is out
                        return kept

                    got, kept = _lidar_guarded(rows, path, call)
                    alive = ~np.isnan(got[:, 0])
                    np.testing.assert_array_equal(alive, want, err_msg=what)
                    TLF._check_filtered(got, rows, alive)
                    assert int(kept.item()) == int(want.sum()), what
                    if kind != "mixed":
                        assert want.all() == (kind == "all_in") and want.any() == (kind == "all_in")
