"""The fp32 convolutions (conv_igemm.hip, conv_winograd.hip, conv_dgrad.hip, conv_wgrad*.hip) through ``ops``, bit for bit
against float64 on the host, with the output and the workspace of every launch between NaN guard bands.

Method.  Operands are small integers held in fp32 (x, w, dy, residual / add, the gradient an accumulating form adds to: [-3, 3];
shift: [-3, 3]; scale / act_scale: {0.5, 1, 2}), so every product, every partial sum and every Winograd transform value is an
integer or a multiple of 1/4 far below 2^24: the float64 result IS the fp32 result, in any summation order, at any K split, on
any tile (F(2x2,3x3): G holds 0, 1, 1/2 -> U = G g G^T is a multiple of 1/4; B^T and A^T hold 0, +-1 -> V, M, Y exact).
``exact_regime`` asserts the precondition per shape on the host.  The comparison is equality with float64, no tolerance.

Buffers.  The output (y / dx / dw / db / the accumulated gradient) and the workspace are views between two NaN bands of BAND
floats; output and workspace are filled with NaN before the call; the workspace has exactly the bytes the library's
``*_ws_bytes`` query answers under the hooks of that form.  After the call: all bands intact, no NaN in the output (an element
never written, or computed from workspace never written), output == float64.  The filter gradient's tile counters are zero again.

A NEW KERNEL FORM (tile index, staging mode, store path, algorithm flag, filter-gradient kernel) MUST BE ADDED TO THE LISTS
BELOW (TILE_INDICES, STAGINGS, STORE_PATHS, WINOGRAD_MODES, WINOGRAD_PLAN_CODES, DGRAD_TILES, WGRAD_KERNELS ...).

Forward kernel reached by (plan tile index, staging mode, C % 32) - resolve_tile in conv_igemm.hip:

    index        C % 32 != 0 (any staging)      staging 0       staging 1          staging 2          staging 3
    0  256x128   launch_reg<4,2,2,2> unaligned  reg aligned     launch_dma<4,2>    launch_dma<4,2>    launch_buf<4,2,2,2>
    1  128x256   launch_reg<2,4,2,2> unaligned  reg aligned     launch_dma<2,4>    launch_dma<2,4>    launch_buf<2,4,2,2>
    2  128x128   launch_reg<2,2,2,2> unaligned  reg aligned     reg aligned        launch_dma2        launch_buf<2,2,2,2>
    3  128x64    launch_reg<2,2,2,1> unaligned  reg aligned     reg aligned        reg aligned        launch_buf<2,2,2,1>
    4  64x128    launch_reg<2,2,1,2> unaligned  reg aligned     reg aligned        reg aligned        launch_buf<2,2,1,2>
    5  64x64     launch_reg<2,2,1,1> unaligned  reg aligned     reg aligned        reg aligned        launch_buf<2,2,1,1>
    6  128x128   launch_reg<2,2,2,2> unaligned  reg aligned     launch_dma2        launch_dma2        launch_dma2
    7  64x64     launch_reg<2,2,1,1> unaligned  reg aligned     launch_buf<2,2,1,1> in modes 1, 2, 3
    8  128x64    launch_reg<2,2,2,1> unaligned  reg aligned     launch_buf<2,2,2,1> in modes 1, 2, 3
    9  64x128    launch_reg<2,2,1,2> unaligned  reg aligned     launch_buf<2,2,1,2> in modes 1, 2, 3
    10 128x128   launch_reg<2,2,2,2> unaligned  reg aligned     launch_buf<2,2,2,2> in modes 1, 2, 3
    11 256x128   launch_reg<4,2,2,2> unaligned  reg aligned     launch_buf<4,2,2,2> in modes 1, 2, 3
    12 128x256   launch_reg<2,4,2,2> unaligned  reg aligned     launch_buf<2,4,2,2> in modes 1, 2, 3
    13 64x64     launch_reg<2,2,1,1> unaligned  reg aligned     launch_pbuf          in modes 1, 2, 3

(all operands here are far below 2 GB, so the "small operand" condition of the buffer-load kernels always holds).  Every shape
but m65_c36_k68, 3x3_one_tile_c8 and stem has C % 32 == 0, so every family is reached by aligned shapes; those three reach the
unaligned register-staged kernels of every tile shape.  The data gradient is a forward convolution of dy, so its "C" is the
layer's K: m65_c36_k68 (68), m259_k132 and 5x5 (132), k260_3steps (260), 3x3s2_even (48), one_pixel and 3x3_one_tile_c8 (4)
run it unaligned.
"""
import contextlib

import pytest

from guarded_buffers import DEV, guarded, guards_flag

BAND = 4096                      # floats per guard band: a one-row overrun of these shapes stays inside the allocation
TWO22 = 1 << 22

# name -> (n, h, w, c, k, r, stride, pad)
SHAPES = {
    "one_pixel": (1, 1, 1, 32, 4, 1, 1, 0),          # M = 1, K = 4: one pixel, one column group, every tile almost empty
    "m65_c36_k68": (1, 5, 13, 36, 68, 1, 1, 0),      # M = 65; C = 36: a full K-step and a tail of 4 (unaligned kernels); K = 68, one over a 64 tile
    "m259_k132": (1, 7, 37, 64, 132, 1, 1, 0),       # M = 259 over the 256 tile, K = 132 over the 128 tile, two K-steps
    "k260_3steps": (1, 3, 5, 96, 260, 1, 1, 0),      # K = 260 over the 256 tile; three K-steps: the split of 2 is ragged
    "3x3_odd_batch": (3, 5, 7, 32, 64, 3, 1, 1),     # image boundaries inside one M tile, padding taps on every side; Winograd: odd H and W, several images
    "3x3_map1": (1, 1, 1, 32, 32, 3, 1, 1),          # a map smaller than the filter
    "3x3_one_tile_c8": (1, 2, 2, 8, 4, 3, 1, 1),     # a single Winograd tile, C % 32 != 0
    "3x3_pad0": (1, 6, 8, 32, 32, 3, 1, 0),          # pad 0: the data gradient pads by 2
    "3x3s2_pad0": (1, 7, 9, 32, 32, 3, 2, 0),        # the same, strided
    "3x3s2_even": (2, 8, 10, 32, 48, 3, 2, 1),       # strided 3x3, even size: a remainder row / column of the zero-inserted map
    "3x3s2_odd": (1, 9, 11, 64, 32, 3, 2, 1),        # strided 3x3, odd size: no remainder
    "1x1s2_even": (1, 6, 8, 64, 32, 1, 2, 0),        # strided 1x1: scattered data gradient, untouched pixels exactly 0 (or `add`)
    "1x1s2_odd": (2, 7, 9, 32, 64, 1, 2, 0),         # the same at odd size, two images
    "stem": (1, 13, 17, 4, 64, 7, 2, 3),             # C = 4 (c_real = 3 in the accumulating filter gradient), 49 taps
    "5x5": (2, 13, 9, 64, 132, 5, 1, 2),             # 5x5, 50 K-steps
    "linear": (37, 1, 1, 1024, 64, 1, 1, 0),         # a Linear layer as a convolution: 32 K-steps, 1x1 maps
    # 33 x 9 tiles of 64x64, 6 K-steps: with 2 splits 594 work items of 3 K-steps each for the persistent kernel's 512 resident
    # workgroups - its K-step stream crosses item and split boundaries (with 1 split 297 items: one each)
    "persistent": (1, 42, 50, 192, 520, 1, 1, 0),
    "layer3": (1, 38, 63, 256, 256, 3, 1, 1),        # one real layer3 shape, through the default (hook-free) path only
}
HOOKED = [name for name in SHAPES if name != "layer3"]

TILE_INDICES = tuple(range(14))
STAGINGS = (0, 1, 2, 3)
STORE_PATHS = (1, 1 | 64)                           # set_conv_algo: implicit GEMM; + stores straight from the MFMA layout
EPILOGUES = ("none", "scale_shift_relu", "scale_shift_residual_relu")
FORCED_TILES = ((4, 2), (2, 4), (2, 2), (2, 1), (1, 2), (1, 1))
WINOGRAD_MODES = tuple(2 | f | t for f in (0, 16, 32) for t in (0, 128))
WINOGRAD_PLAN_CODES = tuple(t + 16 for t in (0, 1, 2, 3, 4, 5, 13)) + (5 + 32,)
DGRAD_TILES = ((0, 0), (1, 1), (2, 2), (4, 2))
DGRAD_STAGINGS = (0, 1, 3)
WGRAD_KERNELS = (1, 2, 3, 4)
WGRAD_SPLITS = (1, 2, 5, 64)

_REF = {}
_DEVICE = {}


# ---- geometry and the exactness precondition ---------------------------------------------------------------------------------
def out_hw(h, w, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1


def winograd_fwd(name):
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    return r == 3 and stride == 1 and pad == 1 and c % 4 == 0 and k % 4 == 0


def ksteps_of(name):
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    return (r * r * c + 31) // 32


def plan_splits(ksteps):
    """(splits, K-steps per split) for splits 1, 2, 3 and ksteps, where ceil(ksteps / steps per split) == splits - the rows
    frcnn_conv2d_import_plans accepts (at most 64 splits)."""
    rows = []
    for sp in (1, 2, 3, ksteps):
        sps = (ksteps + sp - 1) // sp
        if sp <= 64 and (ksteps + sps - 1) // sps == sp and (sp, sps) not in rows:
            rows.append((sp, sps))
    return rows


def exact_regime(name):
    """The precondition of bit-exactness: with |operands| <= 3 a product is at most 9, so every sum the kernels form - the
    convolution times the largest scale, plus shift and residual (3 + 3); the data gradient (K in place of C) times act_scale,
    plus `add`; the filter gradient over the pixels, plus the gradient it is added to (5 covers two accumulations of 3 - 1);
    Winograd: transformed operands up to 9 each - is a multiple of 1/4 below 2^22, hence an fp32 number."""
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = out_hw(h, w, r, stride, pad)
    max_scale = 2
    assert 9 * r * r * c * max_scale + 6 < TWO22, name
    assert 9 * r * r * k * max_scale + 6 < TWO22, name
    assert 9 * n * ho * wo + 5 < TWO22, name
    if winograd_fwd(name):
        assert 81 * r * r * c * max_scale + 6 < TWO22, name
        assert 81 * r * r * k * max_scale + 6 < TWO22, name
    return True


# ---- operands and the float64 reference ------------------------------------------------------------------------------------------
def operands(name):
    import torch
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = out_hw(h, w, r, stride, pad)
    gen = torch.Generator().manual_seed(1000 + list(SHAPES).index(name))
    ints = lambda *shape: torch.randint(-3, 4, shape, generator=gen).double()
    pow2 = lambda count: torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (count,), generator=gen)]
    c_real = 3 if c == 4 else c
    return {
        "x": ints(n, h, w, c), "w": ints(k, r, r, c), "dy": ints(n, ho, wo, k), "residual": ints(n, ho, wo, k),
        "add": ints(n, h, w, c), "scale": pow2(k), "shift": ints(k), "act_scale": pow2(c),
        "act_y": torch.randn((n, h, w, c), generator=gen, dtype=torch.float32).clamp_min(0).double(),
        "before": ints(k, c_real, r, r), "before2": ints(k, c_real, r, r), "before_b": ints(k),
    }


def conv_float64(name, x, wt):
    """The definition: y (n, ho, wo, k) of x (n, h, w, c) and w (k, r, s, c), in the operands' type."""
    import torch.nn.functional as F
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    return F.conv2d(x.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def dx_float64(name, dy, wt):
    """conv_transpose: (n, h, w, c).  Every output pixel's patch of (c, r, s) contributions, folded onto the map."""
    import torch.nn.functional as F
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    cols = dy.reshape(n, -1, k) @ wt.permute(0, 3, 1, 2).reshape(k, c * r * r)       # (n, L, (c, r, s))
    return F.fold(cols.transpose(1, 2), (h, w), (r, r), padding=pad, stride=stride).permute(0, 2, 3, 1).contiguous()


def dw_float64(name, x, dy):
    """sum over output pixels of dy x patch(x): (k, r, s, c)."""
    import torch.nn.functional as F
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    cols = F.unfold(x.permute(0, 3, 1, 2), (r, r), padding=pad, stride=stride)             # (n, c*r*r, L)
    cols = cols.reshape(n, c, r, r, -1).permute(0, 4, 2, 3, 1).reshape(-1, r * r * c)      # (M, (r, s, c))
    return (dy.reshape(-1, k).t() @ cols).reshape(k, r, r, c)


def reference(name):
    """Operands and float64 results of one shape, computed once and left unchanged."""
    if name not in _REF:
        import torch
        ref = operands(name)
        y = conv_float64(name, ref["x"], ref["w"])
        affine = y * ref["scale"] + ref["shift"]
        ref["fwd"] = {"none": y, "scale_shift_relu": torch.relu(affine),
                      "scale_shift_residual_relu": torch.relu(affine + ref["residual"])}
        ref["dx"] = dx_float64(name, ref["dy"], ref["w"])
        ref["dw"] = dw_float64(name, ref["x"], ref["dy"])
        ref["db"] = ref["dy"].reshape(-1, ref["dy"].shape[-1]).sum(0)
        _REF[name] = ref
    return _REF[name]


def dx_wanted(ref, add, act):
    """act in ("none", "y", "y_scale"): dx = act_y > 0 ? (dx [+ add]) * act_scale : 0."""
    import torch
    v = ref["dx"] + ref["add"] if add else ref["dx"]
    if act == "none":
        return v
    return torch.where(ref["act_y"] > 0, v * ref["act_scale"] if act == "y_scale" else v, torch.zeros_like(v))


# Winograd F(2x2, 3x3) on the host, in the operands' type
def winograd_host(x, wt):
    """(U (16,k,c), Y (n,h,w,k)) of x (n,h,w,c), w (k,3,3,c) for stride 1 / pad 1: U = G g G^T, V = B^T d B, M = sum over c of
    the 16 products, Y = A^T M A per 2x2 output tile."""
    import torch
    dt = x.dtype
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=dt)
    Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=dt)
    At = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=dt)
    n, h, w, c = x.shape
    k = wt.shape[0]
    th, tw = (h + 1) // 2, (w + 1) // 2
    xp = torch.zeros((n, 2 * th + 2, 2 * tw + 2, c), dtype=dt)
    xp[:, 1:h + 1, 1:w + 1] = x
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                         # (n, th, tw, c, 4, 4)
    U = torch.einsum("ai,kijc,bj->abkc", G, wt, G)
    V = torch.einsum("ai,ntxcij,bj->abntxc", Bt, d, Bt)
    M = torch.einsum("abntxc,abkc->abntxk", V, U)
    Y = torch.einsum("ia,abntxk,jb->ntixjk", At, M, At).reshape(n, 2 * th, 2 * tw, k)
    return U.reshape(16, k, c), Y[:, :h, :w].contiguous()


# ---- CPU tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_exactness_precondition_holds(name):
    assert exact_regime(name)
    assert plan_splits(ksteps_of(name))[0] == (1, ksteps_of(name))


def test_the_case_table_has_a_ragged_split_and_a_busy_persistent_grid():
    """k260_3steps: 3 K-steps in 2 splits of 2 - the last split has one; persistent: more 64x64 work items than the 512 resident
    workgroups of launch_pbuf at 3 K-steps per item."""
    assert (2, 2) in plan_splits(ksteps_of("k260_3steps")) and ksteps_of("k260_3steps") == 3
    n, h, w, c, k, r, stride, pad = SHAPES["persistent"]
    tiles = ((n * h * w + 63) // 64) * ((k + 63) // 64)
    assert (2, 3) in plan_splits(ksteps_of("persistent")) and tiles * 2 > 512 and tiles < 512


@pytest.mark.parametrize("name", list(SHAPES))
def test_reference_helpers_agree_with_autograd(name):
    """dx_float64 (fold) and dw_float64 (unfold) against torch autograd of F.conv2d in float64: integers, so equal."""
    import torch
    ref = reference(name)
    x, wt = ref["x"].clone().requires_grad_(True), ref["w"].clone().requires_grad_(True)
    y = conv_float64(name, x, wt)
    assert torch.equal(y.detach(), ref["fwd"]["none"])
    y.backward(ref["dy"])
    assert torch.equal(x.grad, ref["dx"])
    assert torch.equal(wt.grad, ref["dw"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_float32_convolution_of_integer_operands_is_exact(name):
    """"Any summation order gives these bits", without a GPU: F.conv2d in float32 on the host equals float64; so do the
    gradients' definitions and the epilogue."""
    import torch
    ref = reference(name)
    f = lambda key: ref[key].float()
    y = conv_float64(name, f("x"), f("w"))
    assert y.dtype == torch.float32 and torch.equal(y.double(), ref["fwd"]["none"])
    assert torch.equal(torch.relu((y * f("scale") + f("shift")) + f("residual")).double(), ref["fwd"]["scale_shift_residual_relu"])
    assert torch.equal(dx_float64(name, f("dy"), f("w")).double(), ref["dx"])
    assert torch.equal(dw_float64(name, f("x"), f("dy")).double(), ref["dw"])
    for key in ("fwd", "dx", "dw"):                                 # and fp32 holds the float64 results
        for t in (ref[key].values() if key == "fwd" else (ref[key],)):
            assert torch.equal(t.float().double(), t)


@pytest.mark.parametrize("name", [s for s in SHAPES if winograd_fwd(s)])
def test_host_winograd_transforms_are_exact_in_float32(name):
    """G g G^T, B^T d B, the 16 products summed over C and A^T M A in float32 equal float64 on the integer operands, and
    float64 equals the direct convolution - for the layer and for its data gradient (dy with the flipped, transposed filter)."""
    import torch
    ref = reference(name)
    flipped = ref["w"].flip(1, 2).permute(3, 1, 2, 0).contiguous()          # (c, r, s, k): conv2d_transpose_filter
    for x, wt, want in ((ref["x"], ref["w"], ref["fwd"]["none"]), (ref["dy"], flipped, ref["dx"])):
        u64, y64 = winograd_host(x, wt)
        u32, y32 = winograd_host(x.float(), wt.float())
        assert y32.dtype == torch.float32
        assert torch.equal(y64, want)
        assert torch.equal(u32.double(), u64) and torch.equal(y32.double(), y64)
        assert torch.equal(u64 * 4, (u64 * 4).round())                       # multiples of 1/4


# ---- guarded device runs ---------------------------------------------------------------------------------------------------------
def lib():
    from faster_rcnn_pytorch_multimodal_amd import _hip
    return _hip.load()


def restore_hooks():
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    _hip.check(lib().frcnn_conv2d_set_tile(0, 0), "set_tile")
    _hip.check(lib().frcnn_conv2d_set_staging(1), "set_staging")
    ops.set_conv_algo(0)
    ops.set_wgrad_plan(0)
    ops.set_wgrad_variant(0)
    _hip.check(lib().frcnn_conv2d_clear_plans(), "clear_plans")


@contextlib.contextmanager
def hooks():
    """Whatever the body sets - tile, staging, algorithm, filter-gradient plan / variant, plan rows - is undone."""
    try:
        yield
    finally:
        restore_hooks()


def set_tile(tm, tn):
    from faster_rcnn_pytorch_multimodal_amd import _hip
    _hip.check(lib().frcnn_conv2d_set_tile(tm, tn), "set_tile")


def set_staging(mode):
    from faster_rcnn_pytorch_multimodal_amd import _hip
    _hip.check(lib().frcnn_conv2d_set_staging(mode), "set_staging")


def import_plans(rows):
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    _hip.check(lib().frcnn_conv2d_clear_plans(), "clear_plans")
    ops.import_conv_plans(rows)


def on_device(name):
    """The shape's operands and float64 results on the device, uploaded once."""
    if name not in _DEVICE:
        import torch
        from faster_rcnn_pytorch_multimodal_amd import ops
        ref = reference(name)
        dev = {key: ref[key].float().to(DEV).contiguous() for key in ("x", "w", "dy", "residual", "add", "scale", "shift", "act_scale", "act_y")}
        dev["fwd"] = {epi: t.to(DEV) for epi, t in ref["fwd"].items()}
        dev["w_t"] = ops.conv2d_transpose_filter(dev["w"])
        torch.cuda.synchronize()
        assert torch.equal(dev["w_t"].cpu().double(), ref["w"].flip(1, 2).permute(3, 1, 2, 0))
        _DEVICE[name] = dev
    return _DEVICE[name]


def floats_of(ws_bytes):
    """The queried workspace as a float count - exactly, never rounded up."""
    assert ws_bytes % 4 == 0, ws_bytes
    return ws_bytes // 4


def verdict(label, obuf, out, wbuf, ws_floats, want):
    """One synchronisation per launch: bands of the output, bands of the workspace, no NaN in the output, output == float64."""
    import torch
    want = want.reshape(-1)
    flags = torch.stack([guards_flag(obuf, out.numel(), BAND), guards_flag(wbuf, ws_floats, BAND), ~torch.isnan(out).any(),
                         (out.double() == want).all()]).tolist()
    assert flags[0], "%s: wrote outside the output" % label
    assert flags[1], "%s: wrote outside the workspace" % label
    if not flags[2]:
        bad = torch.isnan(out).nonzero().reshape(-1)
        pytest.fail("%s: %d of %d output elements are NaN (not written, or computed from workspace never written), first at %d"
                    % (label, bad.numel(), out.numel(), int(bad[0])))
    if not flags[3]:
        bad = (out.double() != want).nonzero().reshape(-1)
        i = int(bad[0])
        pytest.fail("%s: %d of %d output elements differ from float64, first at %d: got %r, want %r"
                    % (label, bad.numel(), out.numel(), i, float(out[i]), float(want[i])))


def run_forward(name, label, epilogue, split_k=0, w_winograd=None):
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = out_hw(h, w, r, stride, pad)
    dev = on_device(name)
    ws_floats = floats_of(int(lib().frcnn_conv2d_fwd_ws_bytes(n, h, w, c, k, r, r, stride, pad, split_k)))   # after the hooks are set
    wbuf, ws = guarded(ws_floats, guard=BAND)
    obuf, out = guarded(n * ho * wo * k, guard=BAND)
    affine = epilogue != "none"
    got = ops.conv2d_nhwc(dev["x"], dev["w"], dev["scale"] if affine else None, dev["shift"] if affine else None,
                          dev["residual"] if epilogue == "scale_shift_residual_relu" else None, stride=stride, pad=pad, relu=affine,
                          split_k=split_k, out=out.view(n, ho, wo, k), ws=ws, w_winograd=w_winograd)
    assert got.data_ptr() == out.data_ptr()
    verdict("%s forward %s %s" % (name, label, epilogue), obuf, out, wbuf, ws_floats, dev["fwd"][epilogue])


def run_dgrad(name, label, add, act, w_winograd=None):
    """Returns False where the library refuses the combination (the strided 1x1 form has no activation epilogue)."""
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    dev = on_device(name)
    if ("dx", add, act) not in dev:
        dev[("dx", add, act)] = dx_wanted(reference(name), add, act).to(DEV)
    ws_floats = floats_of(int(lib().frcnn_conv2d_bwd_data_ws_bytes(n, h, w, c, k, r, r, stride, pad)))
    wbuf, ws = guarded(ws_floats, guard=BAND)
    obuf, out = guarded(n * h * w * c, guard=BAND)
    try:
        got = ops.conv2d_bwd_data(dev["dy"], dev["w_t"], (n, h, w, c), stride=stride, pad=pad, add=dev["add"] if add else None,
                                  w_winograd=w_winograd, act_y=dev["act_y"] if act != "none" else None,
                                  act_scale=dev["act_scale"] if act == "y_scale" else None, out=out.view(n, h, w, c), ws=ws)
    except _hip.HipError as e:
        if "has no activation epilogue" in str(e):
            return False
        raise
    assert got.data_ptr() == out.data_ptr()
    verdict("%s data gradient %s add=%s act=%s winograd filter=%s" % (name, label, add, act, w_winograd is not None), obuf, out, wbuf,
            ws_floats, dev[("dx", add, act)])
    return True


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", HOOKED)
def test_forward_every_tile_staging_split_store_path_and_epilogue(hip, name):
    """Plan rows (installed through import_conv_plans, with and without the residual key) for every tile index x every valid
    split of 1 / 2 / 3 / ksteps, run in staging modes 0 .. 3 with both store paths and the three epilogues; then the six forced
    tiles with the call's split_k argument 0 (the library's choice) .. 3 and the three epilogues."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    assert exact_regime(name)
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    key = [n, h, w, c, k, r, r, stride, pad]
    runs = 0
    with hooks():
        for idx in TILE_INDICES:
            for splits, per_split in plan_splits(ksteps_of(name)):
                import_plans([key + [1, idx, splits, per_split], key + [1 + 256, idx, splits, per_split]])
                assert sorted(row[9:] for row in ops.export_conv_plans()) == [[1, idx, splits, per_split], [1 + 256, idx, splits, per_split]]
                for staging in STAGINGS:
                    set_staging(staging)
                    for algo in STORE_PATHS:
                        ops.set_conv_algo(algo)
                        for epilogue in EPILOGUES:
                            run_forward(name, "plan tile %d, %d x %d K-steps, staging %d, algo %d" % (idx, splits, per_split, staging, algo), epilogue)
                            runs += 1
        import_plans([])
        set_staging(1)
        ops.set_conv_algo(1)
        for tm, tn in FORCED_TILES:
            set_tile(tm, tn)
            for split_k in (0, 1, 2, 3):
                for epilogue in EPILOGUES:
                    run_forward(name, "forced tile (%d, %d), split_k=%d" % (tm, tn, split_k), epilogue, split_k=split_k)
                    runs += 1
    assert runs == (len(TILE_INDICES) * len(plan_splits(ksteps_of(name))) * len(STAGINGS) * len(STORE_PATHS) + len(FORCED_TILES) * 4) * len(EPILOGUES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s for s in HOOKED if winograd_fwd(s)])
def test_forward_winograd_every_mode_and_plan_row(hip, name):
    """Forced Winograd (2; + 16 never fused; + 32 fused where C % 32 == 0; each + 128 untrimmed) with the library's and the
    caller's filter transform, in every staging mode; Winograd plan rows (tile + 16 for tiles 0 .. 5 and 13, 5 + 32 fused)
    under algorithm mode 0 with and without trimming, in every staging mode.  A call with a residual under forced Winograd runs
    the implicit GEMM inside the Winograd-sized workspace."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    assert exact_regime(name)
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    dev = on_device(name)
    u = ops.winograd_filter(dev["w"])
    torch.cuda.synchronize()
    assert torch.equal(u.cpu().double(), winograd_host(reference(name)["x"], reference(name)["w"])[0])
    key = [n, h, w, c, k, r, r, stride, pad]
    with hooks():
        for staging in STAGINGS:
            set_staging(staging)
            for mode in WINOGRAD_MODES:
                ops.set_conv_algo(mode)
                for filt in (None, u):
                    for epilogue in EPILOGUES:
                        run_forward(name, "algo %d, staging %d, caller's filter=%s" % (mode, staging, filt is not None), epilogue, w_winograd=filt)
        for code in WINOGRAD_PLAN_CODES:
            if code == 5 + 32 and c % 32:
                continue                                            # the fused input transform is for C % 32 == 0 (frcnn_hip.h)
            import_plans([key + [1, code, 1, (c + 31) // 32]])
            assert ops.conv_plan_algo(n, h, w, c, k, r, r, stride, pad) == 1
            for staging in STAGINGS:
                set_staging(staging)
                for trim in (0, 128):
                    ops.set_conv_algo(0 | trim)
                    for filt in (None, u):
                        for epilogue in ("none", "scale_shift_relu"):
                            run_forward(name, "plan code %d, staging %d, algo %d, caller's filter=%s" % (code, staging, trim, filt is not None),
                                        epilogue, w_winograd=filt)


# ---- data gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", HOOKED)
def test_data_gradient_every_entry_point_tile_and_staging(hip, name):
    """frcnn_conv2d_bwd_data (plain, with `add`), _act (act_y, act_y + act_scale, each with and without `add`) and _pre (the
    caller's Winograd filter, where the layer is 3x3 / stride 1 / pad 1) under the library's tile and forced tiles (1,1), (2,2),
    (4,2) in staging modes 0, 1, 3 with the implicit GEMM; then the Winograd forms proper (algorithm mode 2 and its flags)."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    assert exact_regime(name)
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    dev = on_device(name)
    wino = r == 3 and stride == 1 and pad == 1
    u_t = ops.winograd_filter(dev["w_t"]) if wino else None
    ran = refused = 0
    with hooks():
        ops.set_conv_algo(1)
        for tm, tn in DGRAD_TILES:
            set_tile(tm, tn)
            for staging in DGRAD_STAGINGS:
                set_staging(staging)
                label = "tile (%d, %d), staging %d" % (tm, tn, staging)
                for add in (False, True):
                    for act in ("none", "y", "y_scale"):
                        if run_dgrad(name, label, add, act):
                            ran += 1
                        else:
                            refused += 1
                        if wino and not add:
                            assert run_dgrad(name, label, add, act, w_winograd=u_t)
        if wino:
            set_tile(0, 0)
            for staging in DGRAD_STAGINGS:
                set_staging(staging)
                for mode in WINOGRAD_MODES:
                    ops.set_conv_algo(mode)
                    for act in ("none", "y", "y_scale"):
                        for filt in (None, u_t):
                            assert run_dgrad(name, "algo %d, staging %d" % (mode, staging), False, act, w_winograd=filt)
                    assert run_dgrad(name, "algo %d, staging %d" % (mode, staging), True, "y_scale")      # `add`: the implicit GEMM
    strided_1x1 = stride > 1 and r == 1
    assert refused == (4 * len(DGRAD_TILES) * len(DGRAD_STAGINGS) if strided_1x1 else 0) and ran + refused == 6 * len(DGRAD_TILES) * len(DGRAD_STAGINGS)


# ---- filter gradient -------------------------------------------------------------------------------------------------------------
def run_wgrad(name, label):
    """One forced plan (or none): the overwriting form with and without the bias gradient, the accumulating form into a
    (k, c_real, r, s) gradient that holds values, with and without a bias gradient that does.  False where the library answers
    that the forced plan does not apply."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ref, dev = reference(name), on_device(name)
    if "dw" not in dev:
        c_real = ref["before"].shape[1]
        dev["dw"], dev["db"] = ref["dw"].to(DEV), ref["db"].to(DEV)
        dev["before"], dev["before_b"] = ref["before"].float().to(DEV), ref["before_b"].float().to(DEV)
        dev["acc"] = (ref["before"] + ref["dw"].permute(0, 3, 1, 2)[:, :c_real]).contiguous().to(DEV)
        dev["acc_b"] = (ref["before_b"] + ref["db"]).to(DEV)
    c_real = dev["before"].shape[1]
    ws_floats = floats_of(int(lib().frcnn_conv2d_bwd_weight_ws_bytes(n, h, w, c, k, r, r, stride, pad)))     # after the plan is forced
    wbuf, ws = guarded(ws_floats, guard=BAND)
    obuf, out = guarded(k * r * r * c, guard=BAND)
    bbuf, bias = guarded(k, guard=BAND)
    try:
        dw, db = ops.conv2d_bwd_weight(dev["x"], dev["dy"], r, r, stride=stride, pad=pad, want_bias=True, out=out.view(k, r, r, c),
                                       out_bias=bias, ws=ws)
    except _hip.HipError as e:
        if "does not apply" in str(e):
            return False
        raise
    assert dw.data_ptr() == out.data_ptr() and db.data_ptr() == bias.data_ptr()
    verdict("%s filter gradient %s" % (name, label), obuf, out, wbuf, ws_floats, dev["dw"])
    verdict("%s bias gradient %s" % (name, label), bbuf, bias, wbuf, ws_floats, dev["db"])
    ws.fill_(float("nan"))
    obuf, out = guarded(k * r * r * c, guard=BAND)
    dw, db = ops.conv2d_bwd_weight(dev["x"], dev["dy"], r, r, stride=stride, pad=pad, want_bias=False, out=out.view(k, r, r, c), ws=ws)
    assert dw.data_ptr() == out.data_ptr() and db is None
    verdict("%s filter gradient without the bias %s" % (name, label), obuf, out, wbuf, ws_floats, dev["dw"])
    ws.fill_(float("nan"))
    obuf, out = guarded(k * c_real * r * r, guard=BAND)
    bbuf, bias = guarded(k, guard=BAND)
    out.copy_(dev["before"].reshape(-1))
    bias.copy_(dev["before_b"])
    ops.conv2d_bwd_weight_acc(dev["x"], dev["dy"], r, r, out.view(k, c_real, r, r), bias, stride=stride, pad=pad, ws=ws)
    verdict("%s accumulated filter gradient %s" % (name, label), obuf, out, wbuf, ws_floats, dev["acc"])
    verdict("%s accumulated bias gradient %s" % (name, label), bbuf, bias, wbuf, ws_floats, dev["acc_b"])
    ws.fill_(float("nan"))
    obuf, out = guarded(k * c_real * r * r, guard=BAND)
    out.copy_(dev["before"].reshape(-1))
    ops.conv2d_bwd_weight_acc(dev["x"], dev["dy"], r, r, out.view(k, c_real, r, r), None, stride=stride, pad=pad, ws=ws)
    verdict("%s accumulated filter gradient without the bias %s" % (name, label), obuf, out, wbuf, ws_floats, dev["acc"])
    return True


def run_wgrad_grouped(name, label):
    """Two layers of one shape in one frcnn_conv2d_bwd_weight_acc_grouped call: (x, dy) into `before`, (-x, dy) into `before2`."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ref, dev = reference(name), on_device(name)
    c_real = ref["before"].shape[1]
    dw = ref["dw"].permute(0, 3, 1, 2)[:, :c_real]
    ws_floats = floats_of(int(lib().frcnn_conv2d_bwd_weight_acc_grouped_ws_bytes(2, c, k, r, r)))
    wbuf, ws = guarded(ws_floats, guard=BAND)
    bufs = [guarded(k * c_real * r * r, guard=BAND) for _ in range(2)]
    for (_, view), before in zip(bufs, (ref["before"], ref["before2"])):
        view.copy_(before.float().reshape(-1).to(DEV))
    x2 = -dev["x"]
    ops.conv2d_bwd_weight_acc_grouped([dev["x"], x2], [dev["dy"], dev["dy"]], r, r, [view.view(k, c_real, r, r) for _, view in bufs],
                                      stride=stride, pad=pad, ws=ws)
    for g, ((buf, view), want) in enumerate(zip(bufs, (ref["before"] + dw, ref["before2"] - dw))):
        verdict("%s grouped filter gradient %s, layer %d" % (name, label, g), buf, view, wbuf, ws_floats, want.contiguous().to(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("name", HOOKED)
def test_filter_gradient_every_kernel_split_and_form(hip, name):
    """set_wgrad_plan(kernel 1 .. 4, 1 / 2 / 5 / 64 pixel splits): overwrite and accumulate into a gradient of c_real channels,
    each with and without the bias gradient; the grouped form under variants 0 (LDS-DMA) and 1 (register-staged).  A plan the library refuses with
    "does not apply" is skipped by that answer - but the register-staged kernels (1, 2) serve every shape."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    assert exact_regime(name)
    served = set()
    with hooks():
        for kernel in WGRAD_KERNELS:
            for splits in WGRAD_SPLITS:
                ops.set_wgrad_plan(kernel, splits)
                if run_wgrad(name, "kernel %d, %d splits" % (kernel, splits)):
                    served.add((kernel, splits))
        ops.set_wgrad_plan(0)
        assert run_wgrad(name, "the library's plan")
        for variant in (0, 1):
            ops.set_wgrad_variant(variant)
            run_wgrad_grouped(name, "variant %d" % variant)
    assert {(kernel, splits) for kernel in (1, 2) for splits in WGRAD_SPLITS} <= served, served
    torch.cuda.synchronize()
    for ring in ops._COUNTER_RINGS.values():
        assert int(ring.ints.abs().max()) == 0, "tile counters are not zero again"


# ---- one real shape, no hooks ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_layer3_shape_through_the_default_path(hip):
    """1 x 38 x 63 x 256 -> 256, 3x3: forward (three epilogues), data gradient (plain; add + mask + scale) and filter gradient
    (both forms, grouped) as the library plans them with no hook set."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    name = "layer3"
    assert exact_regime(name)
    restore_hooks()
    for epilogue in EPILOGUES:
        run_forward(name, "default path", epilogue)
    assert run_dgrad(name, "default path", False, "none") and run_dgrad(name, "default path", True, "y_scale")
    assert run_wgrad(name, "default path")
    run_wgrad_grouped(name, "default path")
    torch.cuda.synchronize()
    for ring in ops._COUNTER_RINGS.values():
        assert int(ring.ints.abs().max()) == 0, "tile counters are not zero again"


# ---- last: nothing is left set ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_hook_is_left_set(hip):
    """Tile (0,0), staging 1, algorithm 0, filter-gradient plan 0 and variant 0: frcnn_settings_signature, which hashes all of
    them, does not change when each is set to its default; the plan cache is empty; a hook-free call still gives float64."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    before = hip.frcnn_settings_signature()
    assert ops.export_conv_plans() == []
    assert hip.frcnn_conv2d_set_tile(0, 0) == 0 and hip.frcnn_conv2d_set_staging(1) == 0
    ops.set_conv_algo(0)
    ops.set_wgrad_plan(0)
    assert hip.frcnn_settings_signature() == before, "a convolution hook was left set"
    ops.set_wgrad_variant(0)                                        # (this one also empties the filter-gradient plan cache)
    assert hip.frcnn_settings_signature() == before, "the filter-gradient variant was left set"
    run_forward("3x3_odd_batch", "hook-free", "scale_shift_residual_relu")
    assert run_wgrad("3x3_odd_batch", "hook-free")
