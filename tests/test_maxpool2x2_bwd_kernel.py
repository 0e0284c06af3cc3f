"""ops.maxpool2x2s2_bwd / frcnn_maxpool2x2s2_bwd (csrc/pool.hip): the gradient of nn.MaxPool2d(2, 2) of the VGG16 body, NHWC
fp32, plain and with the ReLU mask of the convolution in front of the pool (``relu=True``).

The plain reference is CPU autograd of ``torch.nn.functional.max_pool2d``; the ``relu=True`` references are CPU autograd of
``max_pool2d(relu(t))`` with respect to t and the device's own ``act_bwd(maxpool2x2s2_bwd(x, dy), x, relu=True)``.  Routing a
gradient involves no rounding, so every comparison is exact (``==`` on the values - the sign of a zero is not pinned - and NaNs
at the same places).  x and dy lie between guard bands of NaN, dx is a view between sentinel bands and is pre-filled with NaN:
an element the launch did not write shows, and so does a write outside dx.  The trailing row / column of an odd height /
width of x holds NaN: it must come back as exactly 0, which also shows that it was not read.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from test_maxpool2x2_kernel import DEV, SENTINEL, _bands_equal, _guarded

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAX_LANES = 2048 * 256          # FRCNN_MAXPOOL2X2_MAX_LANES: the backward keeps the forward's lane cap (checked below)

# (N, H, W, C).  The last: c4 = 16 and ceil(259 / 2) x ceil(515 / 2) = 130 x 258 cells - 536 640 work items, between one and
# two times the launch's lane cap, so the front lanes walk the grid-stride loop twice; H and W are odd on top of that.
SHAPES = [(1, 2, 2, 4), (1, 3, 5, 4), (2, 7, 9, 12), (1, 4, 6, 260), (1, 259, 515, 64)]
VALUES = np.array([-1.5, -0.5, 0.0, 0.5, 1.0, 2.0], np.float32)        # few values: most windows hold ties


def work_items(shape):
    n, h, w, c = shape
    return n * ((h + 1) // 2) * ((w + 1) // 2) * (c // 4)


def test_grid_stride_shape_lies_between_one_and_two_lane_caps():
    from faster_rcnn_pytorch_multimodal_amd import ops
    header = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    m = re.search(r"#define FRCNN_MAXPOOL2X2_MAX_LANES \((\d+) \* (\d+)\)", header)
    assert m and int(m.group(1)) * int(m.group(2)) == MAX_LANES == ops.MAXPOOL2X2_MAX_LANES
    assert "int frcnn_maxpool2x2s2_bwd(const float* x, const float* dy, float* dx, int n, int h, int w, int c, int relu_mask" in header
    assert MAX_LANES < work_items(SHAPES[-1]) < 2 * MAX_LANES
    assert SHAPES[-1][1] % 2 == 1 and SHAPES[-1][2] % 2 == 1
    assert all(work_items(s) < MAX_LANES for s in SHAPES[:-1])


def test_library_version():
    from faster_rcnn_pytorch_multimodal_amd import _hip
    assert _hip.load().frcnn_version() >= 122


def nchw(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))


def nhwc(t):
    return np.ascontiguousarray(t.numpy().transpose(0, 2, 3, 1))


def reference(x, dy, relu=False):
    """CPU autograd of max_pool2d(2, 2) (``relu``: of max_pool2d(relu(x)) with respect to x), NHWC in and out."""
    import torch
    import torch.nn.functional as F
    t = nchw(x).requires_grad_(True)
    y = F.max_pool2d(F.relu(t) if relu else t, kernel_size=2, stride=2)
    (g,) = torch.autograd.grad(y, t, nchw(dy))
    return nhwc(g)


def run_guarded(x, dy, relu=False):
    """dx of the launch: x and dy between NaN bands, ``out=`` a NaN-filled view between sentinel bands."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    xbuf, xd = _guarded(x, np.nan)
    gbuf, gd = _guarded(dy, np.nan)
    obuf, od = _guarded(np.full(x.shape, np.nan, np.float32), SENTINEL)
    out = ops.maxpool2x2s2_bwd(xd, gd, relu=relu, out=od)
    torch.cuda.synchronize()
    assert out is od
    assert _bands_equal(obuf, od.numel(), SENTINEL), "wrote outside dx"
    assert _bands_equal(xbuf, xd.numel(), np.nan) and _bands_equal(gbuf, gd.numel(), np.nan)
    return od.cpu().numpy()


def tied_input(shape, rng):
    return VALUES[rng.integers(0, len(VALUES), shape)]


def poison_trailing(x):
    n, h, w, c = x.shape
    x = x.copy()
    if h % 2:
        x[:, h - 1] = np.nan
    if w % 2:
        x[:, :, w - 1] = np.nan
    return x


def check_trailing_is_zero(got):
    n, h, w, c = got.shape
    if h % 2:
        assert np.array_equal(got[:, h - 1], np.zeros_like(got[:, h - 1]))
    if w % 2:
        assert np.array_equal(got[:, :, w - 1], np.zeros_like(got[:, :, w - 1]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plain_form_equals_torch_autograd_and_writes_every_element(hip, shape):
    n, h, w, c = shape
    rng = np.random.default_rng(h * 1000 + w)
    x = tied_input(shape, rng)
    dy = rng.standard_normal((n, h // 2, w // 2, c)).astype(np.float32)
    want = reference(x, dy)                                            # torch gives the trailing row / column 0
    got = run_guarded(poison_trailing(x), dy)
    assert not np.isnan(got).any(), "an element of dx was not written (or a NaN outside the windows was read)"
    assert got.shape == x.shape and np.array_equal(got, want)
    check_trailing_is_zero(got)
    # every window routed its dy to exactly one element
    full = got[:, :h // 2 * 2, :w // 2 * 2].reshape(n, h // 2, 2, w // 2, 2, c)
    assert np.array_equal(full.sum(axis=(2, 4)), dy) and np.array_equal((full != 0).sum(axis=(2, 4)), (dy != 0).astype(np.int64))


@pytest.mark.gpu
def test_ties_zeros_infinities_and_nans_follow_torch(hip):
    rng = np.random.default_rng(5)
    shape = (2, 6, 10, 8)
    x = tied_input(shape, rng)
    dy = rng.standard_normal((2, 3, 5, 8)).astype(np.float32)
    x[0, 0:2, 0:2, 0] = [[0.0, -0.0], [-0.0, 0.0]]                      # +-0: equal, the first wins
    x[0, 0:2, 2:4, 0] = [[-0.0, 0.0], [0.0, -0.0]]
    x[0, 2:4, 0:2, 1] = 0.5                                            # all equal
    x[0, 2:4, 2:4, 1] = -np.inf                                        # four -inf: (0,0)
    x[0, 4, 0, 2] = np.inf                                             # +inf wins
    x[0, 4:6, 2:4, 2] = [[1.0, np.inf], [np.inf, 2.0]]                 # two +inf: the first
    x[0, 5, 4, 3] = -np.inf                                            # -inf loses
    for k, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):       # one NaN at each position
        x[1, 0 + a, 2 * k + b, 4] = np.nan
    x[1, 2:4, 0:2, 5] = [[np.nan, 3.0], [np.nan, 1.0]]                 # several NaNs: the last NaN wins
    x[1, 2:4, 2:4, 5] = [[1.0, np.nan], [np.nan, np.inf]]
    x[1, 2:4, 4:6, 5] = [[np.nan, np.nan], [2.0, np.nan]]
    x[1, 4:6, 0:2, 6] = np.nan                                         # all NaN: (1,1)
    x[1, 4:6, 2:4, 6] = [[np.inf, np.nan], [0.0, 0.0]]                 # NaN beats +inf
    want = reference(x, dy)
    got = run_guarded(x, dy)
    assert not np.isnan(got).any()
    assert np.array_equal(got, want)
    # the rule itself, where the issue states it
    assert got[0, 0, 0, 0] == dy[0, 0, 0, 0] and got[0, 0, 2, 0] == dy[0, 0, 1, 0]
    assert got[0, 2, 0, 1] == dy[0, 1, 0, 1] and got[0, 2, 2, 1] == dy[0, 1, 1, 1]
    assert got[0, 4, 3, 2] == dy[0, 2, 1, 2] and got[0, 5, 2, 2] == 0
    assert got[1, 3, 0, 5] == dy[1, 1, 0, 5] and got[1, 3, 2, 5] == dy[1, 1, 1, 5] and got[1, 3, 5, 5] == dy[1, 1, 2, 5]
    assert got[1, 5, 1, 6] == dy[1, 2, 0, 6] and got[1, 4, 3, 6] == dy[1, 2, 1, 6]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_relu_form_equals_autograd_of_pool_of_relu_and_the_unfused_pair(hip, shape):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c = shape
    rng = np.random.default_rng(h * 1000 + w + 1)
    t = tied_input(shape, rng)                                         # finite; half the values <= 0
    t[:, :2, :2] = -1.0                                                # an all-zero window after the ReLU
    x = np.maximum(t, np.float32(0))
    dy = rng.standard_normal((n, h // 2, w // 2, c)).astype(np.float32)
    want = reference(t, dy, relu=True)
    got = run_guarded(poison_trailing(x), dy, relu=True)
    assert not np.isnan(got).any(), "an element of dx was not written"
    assert np.array_equal(got, want)
    check_trailing_is_zero(got)
    assert (x == 0).mean() > 0.3 and np.array_equal(got[:, :2, :2], np.zeros_like(got[:, :2, :2]))
    # the device's own two passes: the plain pool gradient, then the ReLU mask on the full-size tensor
    xd, gd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    pair, _ = ops.act_bwd(ops.maxpool2x2s2_bwd(xd, gd), xd, None, relu=True)
    fused = ops.maxpool2x2s2_bwd(xd, gd, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(fused.view(torch.int32), pair.view(torch.int32)), "the fused form is not bit-equal to the two passes"
    assert np.array_equal(fused.cpu().numpy(), want)


@pytest.mark.gpu
def test_captured_call_holds_no_memset_and_equals_the_eager_one(hip):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model.train_graph import graph_node_kinds
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((2, 9, 13, 20), device=DEV, generator=g).relu_()
    dy = torch.randn((2, 4, 6, 20), device=DEV, generator=g)
    eager = ops.maxpool2x2s2_bwd(x, dy, relu=True)
    dx = torch.empty_like(x)
    ops.maxpool2x2s2_bwd(x, dy, relu=True, out=dx)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        ops.maxpool2x2s2_bwd(x, dy, relu=True, out=dx)
    kinds, nodes, _ = graph_node_kinds(graph)
    assert kinds == {'kernel': 1} and nodes == 1, kinds
    graph.instantiate()
    for _ in range(2):
        dx.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dx, eager)


def test_argument_errors_are_reported_without_a_gpu():
    """Through the C ABI: every bad call returns FRCNN_ERR_ARG on the host, before any launch."""
    from faster_rcnn_pytorch_multimodal_amd import _hip
    lib = _hip.load()
    x, dy, dx = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)      # never dereferenced
    good = dict(x=x, dy=dy, dx=dx, n=1, h=4, w=4, c=8, relu=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.frcnn_maxpool2x2s2_bwd(a["x"], a["dy"], a["dx"], a["n"], a["h"], a["w"], a["c"], a["relu"], None)

    for kw, word in ((dict(c=6), b"c%4==0"), (dict(h=1), b"h>=2"), (dict(w=1), b"w>=2"), (dict(x=None), b"null"),
                     (dict(dy=None), b"null"), (dict(dx=None), b"null"), (dict(n=0), b"n>0"), (dict(c=0), b"bad shape"),
                     (dict(h=-2), b"bad shape"), (dict(x=ctypes.c_void_p(0x10004)), b"16-byte"),
                     (dict(dy=ctypes.c_void_p(0x20008)), b"16-byte"), (dict(dx=ctypes.c_void_p(0x3000c), relu=1), b"16-byte")):
        assert call(**kw) == -1 and word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())
        assert b"maxpool2x2s2_bwd" in lib.frcnn_last_error()


def test_wrapper_refuses_what_is_not_a_device_fp32_nhwc_tensor():
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    with pytest.raises(_hip.HipError, match="no CPU path"):
        ops.maxpool2x2s2_bwd(torch.zeros(1, 4, 4, 4), torch.zeros(1, 2, 2, 4))


@pytest.mark.gpu
def test_wrapper_argument_checks(hip):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    x, dy = torch.zeros((1, 4, 6, 8), device=DEV), torch.zeros((1, 2, 3, 8), device=DEV)
    with pytest.raises(_hip.HipError, match="dy must be"):
        ops.maxpool2x2s2_bwd(x, torch.zeros((1, 2, 2, 8), device=DEV))
    with pytest.raises(_hip.HipError, match="dy must be"):
        ops.maxpool2x2s2_bwd(x, torch.zeros((1, 4, 6, 8), device=DEV))
    with pytest.raises(_hip.HipError, match="out must be"):
        ops.maxpool2x2s2_bwd(x, dy, out=torch.zeros((1, 2, 3, 8), device=DEV))
    with pytest.raises(_hip.HipError, match="contiguous float32"):
        ops.maxpool2x2s2_bwd(x, dy, out=torch.zeros((1, 4, 6, 8), device=DEV, dtype=torch.float64))
    with pytest.raises(_hip.HipError, match=r"c%4==0"):
        ops.maxpool2x2s2_bwd(torch.zeros((1, 4, 6, 6), device=DEV), torch.zeros((1, 2, 3, 6), device=DEV))
    with pytest.raises(_hip.HipError, match="frcnn_maxpool2x2s2_bwd failed"):       # h < 2: dy is empty, the C check refuses
        ops.maxpool2x2s2_bwd(torch.zeros((1, 1, 6, 8), device=DEV), torch.zeros((1, 0, 3, 8), device=DEV))
    # a misaligned pointer: a view that starts one float into its buffer
    buf = torch.zeros(1 * 4 * 6 * 8 + 4, device=DEV)
    with pytest.raises(_hip.HipError, match="16-byte"):
        ops.maxpool2x2s2_bwd(buf[1:1 + 192].view(1, 4, 6, 8), dy)
    with pytest.raises(_hip.HipError, match="16-byte"):
        ops.maxpool2x2s2_bwd(x, dy, out=buf[3:3 + 192].view(1, 4, 6, 8))
