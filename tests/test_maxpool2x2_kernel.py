"""ops.maxpool2x2s2_nhwc / frcnn_maxpool2x2s2_fwd (csrc/pool.hip): nn.MaxPool2d(2, 2) of the VGG16 body, NHWC fp32.

The reference is ``torch.nn.functional.max_pool2d`` on the CPU and the comparison is exact: a maximum has no rounding.
(``==`` on the values: the sign of a zero result is not pinned; NaNs must sit at the same places.)  Every input lies
between two guard bands of NaN and the trailing row / column of an odd height / width is NaN as well - the kernel
propagates NaN, so a read outside the windows shows as a NaN in the output.  Every output is a view into a larger buffer
filled with a sentinel: a write outside it shows.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEV = "cuda:0"
GUARD = 1024
SENTINEL = -12345.5
MAX_LANES = 2048 * 256          # FRCNN_MAXPOOL2X2_MAX_LANES (checked against the header below)

# (N, H, W, C).  The last: c4 = 16 and H // 2 = 129 rows of W // 2 = 257 outputs - 530 448 work items, above the launch's
# MAX_LANES = 524 288 lanes (the kernel's grid cap times its workgroup size), so the lanes at the front of the grid walk their
# grid-stride loop twice and the others once; H and W are odd on top of that.
SHAPES = [(1, 2, 2, 4), (1, 3, 5, 4), (2, 7, 9, 12), (1, 4, 6, 260), (1, 259, 515, 64)]


def test_grid_stride_shape_exceeds_the_lane_count_of_a_launch():
    from faster_rcnn_pytorch_multimodal_amd import ops
    header = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    m = re.search(r"#define FRCNN_MAXPOOL2X2_MAX_LANES \((\d+) \* (\d+)\)", header)
    assert m and int(m.group(1)) * int(m.group(2)) == MAX_LANES == ops.MAXPOOL2X2_MAX_LANES
    n, h, w, c = SHAPES[-1]
    assert MAX_LANES < n * (h // 2) * (w // 2) * (c // 4) < 2 * MAX_LANES
    for n, h, w, c in SHAPES[:-1]:
        assert n * (h // 2) * (w // 2) * (c // 4) < MAX_LANES


def reference(x_nhwc):
    """torch's max_pool2d(2, 2) on the CPU, NHWC in and out."""
    import torch
    import torch.nn.functional as F
    y = F.max_pool2d(torch.from_numpy(np.ascontiguousarray(x_nhwc.transpose(0, 3, 1, 2))), kernel_size=2, stride=2)
    return np.ascontiguousarray(y.numpy().transpose(0, 2, 3, 1))


def _guarded(values, band):
    """``values`` on the device inside a larger buffer, between two GUARD-float bands of ``band``: (buffer, view)."""
    import torch
    flat = np.asarray(values, np.float32).ravel()
    host = np.full(flat.size + 2 * GUARD, band, np.float32)
    host[GUARD:GUARD + flat.size] = flat
    buf = torch.from_numpy(host).to(DEV)
    return buf, buf[GUARD:GUARD + flat.size].view(*np.shape(values))


def _bands_equal(buf, numel, band):
    host = buf.cpu().numpy()
    both = np.concatenate((host[:GUARD], host[GUARD + numel:]))
    return bool(np.isnan(both).all()) if np.isnan(band) else bool(np.all(both == np.float32(band)))


def run_guarded(x):
    """The pool of ``x`` (numpy NHWC) with ``out=`` a view between sentinel bands and x between NaN bands."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c = x.shape
    xbuf, xd = _guarded(x, np.nan)
    ybuf, yd = _guarded(np.full((n, h // 2, w // 2, c), SENTINEL, np.float32), SENTINEL)
    out = ops.maxpool2x2s2_nhwc(xd, out=yd)
    torch.cuda.synchronize()
    assert out is yd                                                   # out= honoured
    assert _bands_equal(ybuf, yd.numel(), SENTINEL), "wrote outside y"
    assert _bands_equal(xbuf, xd.numel(), np.nan)
    return yd.cpu().numpy()


def assert_same(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaNs at other places than torch's"
    keep = ~np.isnan(want)
    assert np.array_equal(got[keep], want[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_torch_and_never_reads_the_trailing_row_and_column(hip, shape):
    n, h, w, c = shape
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.standard_normal(shape).astype(np.float32)
    x[rng.random(shape) < 0.05] = 0.0                                  # ties and zeros among the values
    want = reference(x)
    if h % 2:
        x[:, h - 1] = np.nan
    if w % 2:
        x[:, :, w - 1] = np.nan
    got = run_guarded(x)
    assert not np.isnan(got).any(), "a value outside the windows (or outside x) was read"
    assert got.shape == (n, h // 2, w // 2, c) and np.array_equal(got, want)
    assert not (got == np.float32(SENTINEL)).any(), "an output element was not written"


@pytest.mark.gpu
def test_nan_and_infinities_follow_torch(hip):
    rng = np.random.default_rng(11)
    base = rng.standard_normal((2, 6, 10, 8)).astype(np.float32)
    clean = reference(base)
    for dy in (0, 1):
        for dx in (0, 1):
            for wo in (2, 3):
                x = base.copy()
                x[1, 2 * 1 + dy, 2 * wo + dx, 5] = np.nan
                got = run_guarded(x)
                assert np.isnan(got[1, 1, wo, 5])                      # the window's output is NaN ...
                mask = np.zeros(got.shape, bool)
                mask[1, 1, wo, 5] = True
                assert np.array_equal(got[~mask], clean[~mask])        # ... and nothing else changed
                assert_same(got, reference(x))
    x = base.copy()
    x[0, 0, 0, 0] = np.inf                      # +inf wins its window
    x[0, 2:4, 2:4, 1] = -np.inf                 # a window of -inf only
    x[0, 4, 6, 2] = -np.inf                     # -inf loses
    x[1, 0, 0, 3], x[1, 0, 1, 3] = np.inf, np.nan       # NaN beats +inf
    x[1, 4, 8, 7], x[1, 5, 9, 7] = np.nan, np.nan
    got = run_guarded(x)
    assert got[0, 0, 0, 0] == np.inf and got[0, 1, 1, 1] == -np.inf and np.isfinite(got[0, 2, 3, 2])
    assert np.isnan(got[1, 0, 0, 3]) and np.isnan(got[1, 2, 4, 7]) and int(np.isnan(got).sum()) == 2
    assert_same(got, reference(x))


@pytest.mark.gpu
def test_captured_call_equals_the_eager_one(hip):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((2, 9, 13, 20), device=DEV, generator=g)
    eager = ops.maxpool2x2s2_nhwc(x)
    y = torch.empty_like(eager)
    ops.maxpool2x2s2_nhwc(x, out=y)                                    # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.maxpool2x2s2_nhwc(x, out=y)
    for _ in range(2):
        y.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)
    x.neg_()                                                           # the replay reads the new contents of x
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, ops.maxpool2x2s2_nhwc(x)) and not torch.equal(y, eager)


def test_argument_errors_are_reported_without_a_gpu():
    """Through the C ABI: every bad call returns FRCNN_ERR_ARG on the host, before any launch."""
    from faster_rcnn_pytorch_multimodal_amd import _hip
    lib = _hip.load()
    x, y = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)         # never dereferenced: the checks come first
    good = dict(x=x, y=y, n=1, h=4, w=4, c=8)

    def call(**kw):
        a = dict(good, **kw)
        return lib.frcnn_maxpool2x2s2_fwd(a["x"], a["y"], a["n"], a["h"], a["w"], a["c"], None)

    for kw, word in ((dict(c=6), b"c%4==0"), (dict(h=1), b"h>=2"), (dict(w=1), b"w>=2"), (dict(x=None), b"null"),
                     (dict(y=None), b"null"), (dict(n=0), b"n>0"), (dict(c=0), b"bad shape"), (dict(h=-2), b"bad shape"),
                     (dict(x=ctypes.c_void_p(0x10004)), b"16-byte"), (dict(y=ctypes.c_void_p(0x20008)), b"16-byte")):
        assert call(**kw) == -1 and word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())


def test_wrapper_refuses_what_is_not_a_device_fp32_nhwc_tensor():
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    with pytest.raises(_hip.HipError, match="no CPU path"):
        ops.maxpool2x2s2_nhwc(torch.zeros(1, 4, 4, 4))
