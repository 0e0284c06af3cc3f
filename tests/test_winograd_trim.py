"""Winograd F(2x2, 3x3) without the transform components that feed only dropped outputs (csrc/conv_winograd.hip, wino_geom).

A map with odd height has a last row of 2x2 output tiles whose second output row lies outside the map; component row i = 3
of such a tile enters nothing else, and likewise column j = 3 in the last tile column of a map with odd width.  By default
those components are neither transformed nor multiplied: the planes of the grouped GEMM hold their tiles class-major
[interior | right edge | bottom edge | corner] and the groups have their own row counts.  frcnn_conv2d_set_algo flag 128
turns the trimming off; every surviving value is computed exactly as before, so the two forms must agree bit for bit.

GPU: each case runs under set_conv_algo(2) and set_conv_algo(2 | 128) with the same GEMM tile, with the library workspace
(and, where the wrapper takes one, the output tensor) filled with NaN before the call: a read of a V or M row the call did
not write, or an output left unwritten, shows as a NaN or as a difference.  The GEMM tile is forced the way a tuned table
forces it - an imported Winograd plan row of the call's shape, which forced mode 2 runs (frcnn_conv2d_set_tile itself puts a
forced-mode call on the implicit GEMM, so it cannot select the tile of the Winograd GEMM).
CPU: frcnn_conv2d_winograd_rows against the class formulas, the workspace size and the version.
Every test leaves the plan cache empty, algorithm mode 0 and staging mode 1.
"""
import contextlib

import pytest
import torch

from faster_rcnn_pytorch_multimodal_amd import _hip, ops

DEV = "cuda:0"
NO_TRIM = 128
NUM_TILES = 14                      # plan tile indices 0 .. 13 (kTiles in conv_igemm.hip)
TILE_64, TILE_128 = 5, 2            # the two tiles forced Winograd picks itself (below / from 2048 GEMM rows)

SHAPES = [
    (3, 7, 7, 32, 64),              # both dimensions odd
    (37, 7, 7, 32, 32),             # class boundaries (333 | 444 | 555 | 592 rows) straddle 64- and 128-row tiles
    (2, 5, 6, 32, 64),              # H odd only
    (1, 4, 9, 32, 64),              # W odd only
    (3, 1, 1, 32, 32),              # corner class only: three component kinds have zero rows
    (2, 1, 6, 32, 32),              # bottom class only
    (2, 6, 1, 32, 32),              # right class only
    (1, 3, 3, 8, 4),                # unaligned kernel (C % 32 != 0), K below a tile
    (2, 6, 8, 32, 64),              # even x even: the identity case
]
VARIED = SHAPES[:2]


def _expected_rows(n, h, w, trim=True):
    th, tw = (h + 1) // 2, (w + 1) // 2
    eh, ew = (h & 1, w & 1) if trim else (0, 0)
    fh, fw = th - eh, tw - ew
    n_i, n_r, n_b = n * fh * fw, n * fh * ew, n * eh * fw
    t = n * th * tw
    rows = [t, n_i + n_r, n_i + n_b, n_i]
    return rows, 9 * rows[0] + 3 * rows[1] + 3 * rows[2] + rows[3]


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_winograd_rows_follow_the_class_formulas():
    try:
        ops.set_conv_algo(0)
        assert ops.winograd_rows(300, 7, 7) == ([4800, 3600, 3600, 2700], 67500)
        for n, h, w in [(300, 7, 7), (1, 38, 63), (1, 75, 125), (1, 1, 1), (2, 1, 6), (2, 6, 1), (37, 7, 7), (2, 5, 6)]:
            assert ops.winograd_rows(n, h, w) == _expected_rows(n, h, w), (n, h, w)
        assert ops.winograd_rows(1, 1, 1) == ([1, 0, 0, 0], 9)
        t = 2 * 3 * 4
        assert ops.winograd_rows(2, 6, 8) == ([t] * 4, 16 * t)                    # even map: nothing to trim
        for mode in (0, 2, 2 | 16):                                                # trimmed in every mode ...
            ops.set_conv_algo(mode)
            assert ops.winograd_rows(300, 7, 7)[1] == 67500, mode
        for mode in (NO_TRIM, 2 | NO_TRIM, 2 | 16 | NO_TRIM):                      # ... unless the flag is set
            ops.set_conv_algo(mode)
            assert ops.winograd_rows(300, 7, 7) == ([4800] * 4, 16 * 4800), mode
            assert ops.winograd_rows(1, 38, 63) == _expected_rows(1, 38, 63, trim=False)
        assert _hip.load().frcnn_conv2d_winograd_rows(0, 7, 7, None) == 0          # bad shape; NULL out is allowed
    finally:
        ops.set_conv_algo(0)


def test_winograd_workspace_is_unchanged_by_the_flag():
    lib = _hip.load()
    up = lambda v: -(-v // 256) * 256
    try:
        for n, h, w, c, k in [(300, 7, 7, 512, 512), (3, 7, 7, 32, 64), (1, 38, 63, 256, 256), (3, 1, 1, 32, 32)]:
            t = n * ((h + 1) // 2) * ((w + 1) // 2)
            want = up(16 * k * c * 4) + up(16 * t * c * 4) + up(16 * t * k * 4)
            got = []
            for mode in (2, 2 | NO_TRIM):
                ops.set_conv_algo(mode)
                got.append(int(lib.frcnn_conv2d_fwd_ws_bytes(n, h, w, c, k, 3, 3, 1, 1, 0)))
            assert got == [want, want], (n, h, w, c, k, got, want)
    finally:
        ops.set_conv_algo(0)


def test_version_and_flag_validation():
    lib = _hip.load()
    assert lib.frcnn_version() >= 117
    try:
        assert lib.frcnn_conv2d_set_algo(2 | NO_TRIM) == 0
        assert lib.frcnn_conv2d_set_algo(256) != 0                                 # the next bit is still refused
    finally:
        ops.set_conv_algo(0)


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _nan_workspace(monkeypatch):
    """ops._workspace hands every call a buffer of 0xFF bytes (as float32: NaN).  Yields the list of sizes handed out."""
    handed = []

    def poisoned(nbytes, device):
        handed.append(int(nbytes))
        return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=device)

    with monkeypatch.context() as m:
        m.setattr(ops, "_workspace", poisoned)
        yield handed


def _reset(lib):
    _hip.check(lib.frcnn_conv2d_set_staging(1), "set_staging")
    _hip.check(lib.frcnn_conv2d_clear_plans(), "clear_plans")
    ops.set_conv_algo(0)


def _tensors(shape, dgrad=False):
    n, h, w, c, k = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * w + n)
    x = torch.randn(n, h, w, c, generator=g).to(DEV)
    wt = (torch.randn(k, 3, 3, c, generator=g) / (3.0 * c ** 0.5)).to(DEV)
    sc, sh = (torch.rand(k, generator=g) + 0.5).to(DEV), torch.randn(k, generator=g).to(DEV)
    if not dgrad:
        return x, wt, sc, sh
    dy = torch.randn(n, h, w, k, generator=g).to(DEV)
    act_y = torch.randn(n, h, w, c, generator=g).to(DEV)        # about half the mask is off
    act_scale = (torch.rand(c, generator=g) + 0.5).to(DEV)
    return dy, ops.conv2d_transpose_filter(wt), act_y, act_scale


def _plan_row(shape, tile, dgrad=False):
    """A Winograd plan row of the forward call of `shape` (of its data-gradient convolution: channels swapped)."""
    n, h, w, c, k = shape
    cin, cout = (k, c) if dgrad else (c, k)
    return [n, h, w, cin, cout, 3, 3, 1, 1, 1, tile + 16, 1, -(-cin // 32)]


def _both_forms(call, handed):
    """call() under forced Winograd, trimmed and untrimmed: finite and equal.  Returns the trimmed result."""
    got = []
    for mode in (2, 2 | NO_TRIM):
        ops.set_conv_algo(mode)
        before = len(handed)
        got.append(call())
        assert len(handed) > before and handed[-1] > 16, "the call took no workspace: it did not run as Winograd"
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got[0]).all()), "trimmed form: a value that the call did not compute reached the output"
    assert bool(torch.isfinite(got[1]).all())
    assert torch.equal(got[0], got[1]), "trimmed form differs: max %.3e" % float((got[0] - got[1]).abs().max())
    return got[0]


def _fwd_call(x, wt, sc, sh, u=None):
    n, h, w, _ = x.shape

    def call():
        out = torch.full((n, h, w, wt.shape[0]), float("nan"), device=DEV)
        return ops.conv2d_nhwc(x, wt, sc, sh, stride=1, pad=1, relu=True, out=out, w_winograd=u)
    return call


def _dgrad_call(dy, w_t, x_shape, u, act_y, act_scale):
    def call():
        poison = torch.full(tuple(x_shape), float("nan"), device=DEV)      # the block dx is most likely carved from
        del poison
        return ops.conv2d_bwd_data(dy, w_t, x_shape, stride=1, pad=1, w_winograd=u, act_y=act_y, act_scale=act_scale)
    return call


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_trimmed_winograd_is_bit_identical(hip, monkeypatch, shape):
    """Every shape on the two GEMM tiles forced Winograd would pick, and within rounding of the implicit GEMM."""
    x, wt, sc, sh = _tensors(shape)
    try:
        with _nan_workspace(monkeypatch) as handed:
            outs = []
            for tile in (TILE_64, TILE_128):
                _hip.check(hip.frcnn_conv2d_clear_plans(), "clear_plans")
                ops.import_conv_plans([_plan_row(shape, tile)])
                outs.append(_both_forms(_fwd_call(x, wt, sc, sh), handed))
            assert torch.equal(outs[0], outs[1])                                   # tile independent
            ops.set_conv_algo(1)
            direct = ops.conv2d_nhwc(x, wt, sc, sh, stride=1, pad=1, relu=True)
        scale = float(direct.abs().max())
        assert float((outs[0] - direct).abs().max()) <= 1e-5 * scale
    finally:
        _reset(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("staging", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", VARIED, ids=lambda s: "x".join(map(str, s)))
def test_trimmed_winograd_on_every_tile_and_staging_mode(hip, monkeypatch, shape, staging):
    """Every plan tile index (all six tile shapes on the register-staged, LDS-DMA and buffer-load kernels; index 13, the
    persistent kernel, runs untrimmed) in every staging mode: trimmed == untrimmed, and one result for all of them."""
    x, wt, sc, sh = _tensors(shape)
    try:
        _hip.check(hip.frcnn_conv2d_set_staging(staging), "set_staging")
        with _nan_workspace(monkeypatch) as handed:
            outs = []
            for tile in range(NUM_TILES):
                _hip.check(hip.frcnn_conv2d_clear_plans(), "clear_plans")
                ops.import_conv_plans([_plan_row(shape, tile)])
                outs.append(_both_forms(_fwd_call(x, wt, sc, sh), handed))
        for tile, o in enumerate(outs):
            assert torch.equal(o, outs[0]), "tile %d" % tile
    finally:
        _reset(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", VARIED, ids=lambda s: "x".join(map(str, s)))
def test_trimmed_winograd_with_a_supplied_filter_and_as_data_gradient(hip, monkeypatch, shape):
    """frcnn_conv2d_fwd_pre (w_winograd supplied) and the data-gradient entry with a Winograd filter, without and with the
    activation-backward epilogue (act_y / act_scale), on both tiles."""
    n, h, w, c, k = shape
    x, wt, sc, sh = _tensors(shape)
    dy, w_t, act_y, act_scale = _tensors(shape, dgrad=True)
    u, u_t = ops.winograd_filter(wt), ops.winograd_filter(w_t)
    try:
        with _nan_workspace(monkeypatch) as handed:
            for tile in (TILE_64, TILE_128):
                _hip.check(hip.frcnn_conv2d_clear_plans(), "clear_plans")
                ops.import_conv_plans([_plan_row(shape, tile), _plan_row(shape, tile, dgrad=True)])
                pre = _both_forms(_fwd_call(x, wt, sc, sh, u), handed)
                assert torch.equal(pre, _both_forms(_fwd_call(x, wt, sc, sh), handed))
                plain = _both_forms(_dgrad_call(dy, w_t, (n, h, w, c), u_t, None, None), handed)
                act = _both_forms(_dgrad_call(dy, w_t, (n, h, w, c), u_t, act_y, act_scale), handed)
                torch.cuda.synchronize()
                assert torch.equal(act, torch.where(act_y > 0, plain * act_scale, torch.zeros_like(plain)))
                masked = _both_forms(_dgrad_call(dy, w_t, (n, h, w, c), u_t, act_y, None), handed)
                assert torch.equal(masked, torch.where(act_y > 0, plain, torch.zeros_like(plain)))
    finally:
        _reset(hip)


@pytest.mark.gpu
def test_imported_plan_runs_trimmed_in_mode_0(hip, monkeypatch):
    """The path the benchmark takes: a Winograd row of an imported table under mode 0 (tile 6, the two-stage LDS-DMA
    128x128 kernel) against forced, untrimmed Winograd without a table."""
    shape = (64, 7, 7, 256, 256)
    row = [64, 7, 7, 256, 256, 3, 3, 1, 1, 1, 22, 1, 8]
    x, wt, sc, sh = _tensors(shape)
    try:
        with _nan_workspace(monkeypatch) as handed:
            ops.set_conv_algo(2 | NO_TRIM)
            ref = _fwd_call(x, wt, sc, sh)()
            ops.set_conv_algo(0)
            ops.import_conv_plans([row])
            assert ops.conv_plan_algo(*row[:9]) == 1
            assert ops.winograd_rows(64, 7, 7)[1] < 16 * 64 * 16
            got = _fwd_call(x, wt, sc, sh)()
            assert len(handed) == 2 and min(handed) > 16
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all())
        assert torch.equal(got, ref), "max %.3e" % float((got - ref).abs().max())
    finally:
        _reset(hip)
