"""cfg.TEST.CONV_SPLIT_BF16: fp32-accurate forward convolutions on the bf16 matrix pipe (frcnn_conv2d_fwd_bf16x3,
DESIGN 4.20).  Every fp32 operand is hi + mid + lo, three bf16 values; a product is six bf16 products accumulated in fp32.

CPU: the split and the six-product arithmetic in torch, the switch, the dispatch, the frame-graph key, the wrappers'
argument checks.  GPU: the kernel at the smallest shapes where it can go wrong (rule tile and both forced tiles, bit-equal),
exact results on integer operands, the error against float64 set against the fp32 kernel's own (gate 1 of
profiles/conv_split_bf16.md), the operand range, the switch through the ResNet-101 detector and a captured frame."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bench
from faster_rcnn_pytorch_multimodal_amd import _hip, ops
from faster_rcnn_pytorch_multimodal_amd.model import config as C
from faster_rcnn_pytorch_multimodal_amd.nets import hip_modules as H

DEV = "cuda:0"
# (n, h, w, c, k, r, s, stride, pad), with / without scale, shift, residual and ReLU
SMALL = [((2, 5, 7, 32, 40, 1, 1, 1, 0), False),       # one K-step, M and N tails
         ((1, 9, 11, 64, 72, 3, 3, 1, 1), False),      # padding taps, K-steps across taps
         ((1, 8, 8, 96, 136, 1, 1, 2, 0), False),      # stride 2
         ((3, 7, 7, 64, 64, 3, 3, 1, 1), True),        # scale, shift, residual, ReLU
         ((1, 6, 6, 288, 64, 1, 1, 1, 0), False)]      # nine K-steps
# the four large GEMMs of the 1000 x 600 frame; the rule takes the three 1x1 ones and leaves the 3x3 to fp32 Winograd
FRAME = [(300, 7, 7, 2048, 512, 1, 1, 1, 0), (300, 7, 7, 512, 2048, 1, 1, 1, 0), (300, 7, 7, 512, 512, 3, 3, 1, 1),
         (1, 38, 63, 1024, 2560, 1, 1, 1, 0)]
TILES = (0, 1, 2)
GATE = 1.25          # the split kernel's error may exceed the fp32 kernel's by a quarter (another summation order, random data)
# Measured on an MI355X, recorded in profiles/conv_split_bf16.md (ResNet-101 image detector, 192x320 frame, seed 5 / frame 7):
# switch on against switch off.  The bounds below are 4 x these, the head-room tests/test_conv_bf16.py gives its own gaps.
CLS_PROB_MAX_ABS, BBOX_PRED_MAX_ABS = 2.98e-8, 2.027e-6


def shape_id(sh):
    sh = sh[0] if isinstance(sh[0], tuple) else sh
    return "n%d_%dx%d_c%d_k%d_%dx%d_s%d_p%d" % sh


def conv64(x_nhwc, w_krsc, stride, pad):
    """float64 convolution on the host: NHWC input, KRSC filter -> NHWC output."""
    y = F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w_krsc.double().permute(0, 3, 1, 2), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


def out_shape(sh):
    n, h, w, c, k, r, s, stride, pad = sh
    return n, (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1, k


def bf16_round(t):
    return t.to(torch.bfloat16).float()


def split3(t):
    """The reference split in torch (round to nearest even): hi = bf16(t), mid = bf16(t - hi), lo = bf16(t - hi - mid)."""
    hi = bf16_round(t)
    r1 = t - hi
    mid = bf16_round(r1)
    return hi, mid, bf16_round(r1 - mid)


SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # (x plane, w plane), smallest first: the kernel's order


def six_products(x, w, group=None, two=False):
    """x (M, K) @ w (K, N) from the six plane products, smallest first, fp32 accumulation (a bf16 product is exact in fp32, so
    each fp32 matmul of two planes is an fp32 sum of exact products).  ``group``: None = six whole matmuls added up; 16 = the
    kernel's k order, the six terms of one k-group of 16 after those of the group before.  ``two``: the kernel's two
    accumulators - the five small terms in one, hi*hi in the other, added once at the end - instead of one."""
    xs, ws = split3(x), split3(w)
    acc = torch.zeros(x.shape[0], w.shape[1])
    low = torch.zeros_like(acc)
    for g in range(0, x.shape[1], group or x.shape[1]):
        for t, (a, b) in enumerate(SIX):
            to = low if (two and t < 5) else acc
            to += xs[a][:, g:g + (group or x.shape[1])] @ ws[b][g:g + (group or x.shape[1])]
    return acc + low


def dev(t):
    return None if t is None else t.to(DEV)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_split3_is_exact():
    g = torch.Generator().manual_seed(0)
    rnd = torch.cat([torch.randn(20000, generator=g) * s for s in (1.0, 1e-3, 50.0, 1e10, 1e-20)])
    pow2 = torch.tensor([2.0 ** e for e in range(-100, 101)])
    pow2 = torch.cat([pow2, -pow2])
    ones = torch.tensor([0x3FFFFFFF, 0x3F7FFFFF, 0x4B7FFFFF, 0xBFFFFFFF, 0x00FFFFFF | (60 << 23), 0x007FFFFF | (200 << 23)],
                        dtype=torch.int64).to(torch.int32).view(torch.float32)          # all 24 significant bits set
    for t in (rnd, pow2, ones):
        hi, mid, lo = split3(t)
        assert torch.equal((hi + mid) + lo, t) and torch.equal(hi.double() + mid.double() + lo.double(), t.double())
    hi, mid, lo = split3(torch.tensor([1 + 2.0 ** -7 + 2.0 ** -15 + 2.0 ** -23]))      # ties in both remainders go to even
    assert (float(hi), float(mid), float(lo)) == (1 + 2.0 ** -7, 2.0 ** -15, 2.0 ** -23)
    hi, mid, lo = split3(pow2)
    assert torch.equal(hi, pow2) and not mid.any() and not lo.any()


@pytest.mark.parametrize("K", [512, 2048])
def test_six_products_are_at_or_below_the_fp32_matmul_error(K):
    """Post-ReLU normal activations, normal filters x 0.05; largest error against float64 relative to the largest output.
    Expectation (the emulation the kernel was specified from): fp32 2.8e-7 / 2.5e-7, six products 1.5e-7 / 1.3e-7, three
    products (hi*hi, hi*mid, mid*hi) 4.9e-6 / 4.4e-6 at K = 512 / 2048.  The matmuls are torch's, which sum in blocks; the
    kernel adds its MFMA results one after the other, group after group, the five small terms and hi*hi in accumulators
    of their own, as the fp32 kernel adds K / 2 results - that order costs both of them accuracy against a blocked sum
    (printed for one and for two accumulators, not asserted here: torch's fp32 adds round to nearest, the MFMA's do not)
    and is judged on the device, kernel against kernel (the gate tests below)."""
    g = torch.Generator().manual_seed(K)
    x = torch.randn((192, K), generator=g).clamp(min=0)
    w = torch.randn((K, 160), generator=g) * 0.05
    ref = x.double() @ w.double()
    top = float(ref.abs().max())
    e32 = float((x @ w - ref).abs().max()) / top
    e6 = float((six_products(x, w) - ref).abs().max()) / top
    xs, ws = split3(x), split3(w)
    e3 = float(((xs[1] @ ws[0] + xs[0] @ ws[1]) + xs[0] @ ws[0] - ref).abs().max()) / top
    e6seq = float((six_products(x, w, 16) - ref).abs().max()) / top
    e6two = float((six_products(x, w, 16, two=True) - ref).abs().max()) / top
    print("K %d: fp32 %.3g, six products %.3g (group after group: one accumulator %.3g, the kernel's two %.3g), three products %.3g"
          % (K, e32, e6, e6seq, e6two, e3))
    assert e6 <= e32
    assert e6 < 4e-7 and e3 > 4 * e6          # six reach fp32, three do not


def test_switch_is_on_by_default():
    C.reset_cfg()
    assert C.cfg.TEST.CONV_SPLIT_BF16 is True and C.cfg.TEST.CONV_BF16 is False


def test_rule_selects_the_large_gemms_and_yields_to_the_fp32_hooks():
    lib = _hip.load()
    try:
        for sh in FRAME:
            assert ops.conv_split_bf16_wanted(*sh) is (sh[5] == 1)
        assert ops.conv_split_bf16_wanted(600, 7, 7, 512, 512, 3, 3, 2, 1) is True          # no Winograd form at stride 2
        for sh, _ in SMALL:
            assert ops.conv_split_bf16_wanted(*sh) is False
        # the frame's other layers: short K, narrow N, or fewer 128x128 tiles than CUs
        for sh in ((1, 38, 63, 256, 1024, 1, 1, 1, 0), (1, 38, 63, 1024, 256, 1, 1, 1, 0), (1, 38, 63, 256, 256, 3, 3, 1, 1),
                   (1, 38, 63, 1024, 512, 3, 3, 1, 1), (1, 75, 125, 512, 128, 1, 1, 1, 0), (1, 150, 250, 64, 256, 1, 1, 1, 0),
                   (300, 7, 7, 2048, 512, 1, 1, 1, 0)[:3] + (2040, 512, 1, 1, 1, 0)):          # C % 32 != 0
            assert ops.conv_split_bf16_wanted(*sh) is False
        big = FRAME[0]
        assert lib.frcnn_conv2d_set_tile(2, 2) == 0 and ops.conv_split_bf16_wanted(*big) is False
        assert lib.frcnn_conv2d_set_tile(0, 0) == 0 and ops.conv_split_bf16_wanted(*big) is True
        for mode in (1, 2, 16, 64, 128):
            ops.set_conv_algo(mode)
            assert ops.conv_split_bf16_wanted(*big) is False
        ops.set_conv_algo(0)
        assert ops.conv_split_bf16_wanted(*big) is True
        sig = lib.frcnn_settings_signature()
        assert lib.frcnn_conv2d_split_bf16_enable(0) == 0 and ops.conv_split_bf16_wanted(*big) is False
        assert lib.frcnn_settings_signature() != sig
        assert lib.frcnn_conv2d_split_bf16_enable(2) != 0
        assert lib.frcnn_conv2d_split_bf16_enable(1) == 0 and lib.frcnn_settings_signature() == sig
    finally:
        lib.frcnn_conv2d_set_tile(0, 0)
        ops.set_conv_algo(0)
        lib.frcnn_conv2d_split_bf16_enable(1)


def test_dispatch_truth_table(monkeypatch):
    """``conv_forward`` on host tensors: switch x net mode x gradient x eligibility x CONV_BF16 precedence."""
    C.reset_cfg()
    taken = []
    monkeypatch.setattr(ops, "conv2d_nhwc", lambda *a, **kw: taken.append("fp32"))
    monkeypatch.setattr(ops, "conv2d_nhwc_bf16", lambda *a, **kw: taken.append("bf16"))
    monkeypatch.setattr(ops, "conv2d_nhwc_bf16x3", lambda *a, **kw: taken.append("split"))
    monkeypatch.setattr(H, "_bf16_entry", lambda holder, name, w, pack=None: (name, pack))
    n, h, w, c, k = FRAME[1][:5]
    big_x, big_w = torch.zeros(n, h, w, c), torch.zeros(k, 1, 1, c)
    small_x, small_w = torch.zeros(1, 4, 4, 32), torch.zeros(8, 3, 3, 32)
    odd_x, odd_w = torch.zeros(n, h, w, 520), torch.zeros(k, 1, 1, 520)          # C % 32 != 0

    def route(x, wt, pad=0):
        del taken[:]
        H.conv_forward(x, wt, None, None, None, object(), stride=1, pad=pad)
        assert len(taken) == 1
        return taken[0]
    try:
        for split in (False, True):
            for bf16 in (False, True):
                for mode in (None, "TRAIN", "TEST"):
                    C.cfg.TEST.CONV_SPLIT_BF16, C.cfg.TEST.CONV_BF16 = split, bf16
                    H.set_net_mode(mode)
                    test = mode == "TEST"
                    with torch.no_grad():
                        assert route(big_x, big_w) == ("bf16" if bf16 and test else "split" if split and test else "fp32")
                        assert route(small_x, small_w, pad=1) == ("bf16" if bf16 and test else "fp32")      # the rule says no
                        assert route(odd_x, odd_w) == "fp32"
                        assert H.conv_split_bf16_wanted(big_x, big_w, 1, 0) is (split and test)
                    assert route(big_x.clone().requires_grad_(True), big_w) == "fp32"                       # a gradient is wanted
    finally:
        H.set_net_mode(None)
        C.reset_cfg()


def test_frame_graph_key_carries_the_switch():
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import cfg_fingerprint
    C.reset_cfg()
    net = torch.nn.Sequential(torch.nn.Conv2d(4, 4, 1))
    try:
        on = cfg_fingerprint(net)
        C.cfg.TEST.CONV_SPLIT_BF16 = False
        off = cfg_fingerprint(net)
        C.cfg.TEST.CONV_SPLIT_BF16 = True
        assert cfg_fingerprint(net) == on and on != off
        assert sum(a != b for a, b in zip(on, off)) == 1
    finally:
        C.reset_cfg()


def test_wrappers_reject_bad_arguments_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_hip, "load", no_library)
    x = torch.zeros(1, 4, 4, 32)
    w16 = torch.zeros(3, 8, 1, 1, 32, dtype=torch.int16)
    with pytest.raises(_hip.HipError):
        ops.conv2d_pack_bf16x3(torch.zeros(8, 1, 1, 32))                                 # CPU tensor
    with pytest.raises(_hip.HipError):
        ops.conv2d_pack_bf16x3(torch.zeros(8, 1, 1, 32, dtype=torch.float64))
    with pytest.raises(_hip.HipError):
        ops.conv2d_nhwc_bf16x3(x, w16)                                                   # CPU tensors
    for bad in ((0, 7, 7, 64, 64, 1, 1, 1, 0), (1, 7, 7, 64, 64, 1, 1, 0, 0), (1, 7, 7, 64, 64, 1, 1, 1, -1)):
        with pytest.raises(_hip.HipError):
            ops.conv_split_bf16_wanted(*bad)

    class OnDevice(torch.Tensor):       # a host tensor that claims to be on the device: reaches the shape / dtype checks
        is_cuda = True

    def fake(t):
        return t.as_subclass(OnDevice)
    good_x, good_w = fake(x), fake(w16)
    bad = [(fake(torch.zeros(1, 4, 4, 48)), fake(torch.zeros(3, 8, 1, 1, 48, dtype=torch.int16)), {}),    # C % 32 != 0
           (fake(torch.zeros(1, 4, 4, 64)), good_w, {}),                                                  # channel mismatch
           (good_x, fake(torch.zeros(3, 8, 1, 1, 32)), {}),                                               # fp32 filter
           (good_x, fake(torch.zeros(8, 1, 1, 32, dtype=torch.int16)), {}),                               # one plane
           (good_x, fake(torch.zeros(2, 8, 1, 1, 32, dtype=torch.int16)), {}),                            # two planes
           (fake(torch.zeros(4, 4, 32)), good_w, {}),                                                     # x not 4-D
           (good_x, fake(torch.zeros(3, 8, 5, 5, 32, dtype=torch.int16)), {}),                            # filter larger than the map
           (good_x, good_w, {"stride": 0}), (good_x, good_w, {"pad": -1}),
           (good_x, good_w, {"scale": fake(torch.zeros(7))}), (good_x, good_w, {"shift": fake(torch.zeros(9))}),
           (good_x, good_w, {"residual": fake(torch.zeros(1, 4, 4, 4))}),
           (good_x, good_w, {"out": fake(torch.zeros(1, 4, 4, 4))})]
    for bx, bw, kw in bad:
        with pytest.raises(_hip.HipError):
            ops.conv2d_nhwc_bf16x3(bx, bw, **kw)
    with pytest.raises(_hip.HipError):
        ops.conv2d_pack_bf16x3(fake(torch.zeros(8, 32)))


# ---- GPU: the kernel ------------------------------------------------------------------------------------------------------
def run_split(x, w_packed, scale, shift, res, sh, relu, tile):
    ops.set_conv_bf16_tile(tile)
    try:
        y = ops.conv2d_nhwc_bf16x3(x, w_packed, scale, shift, res, stride=sh[7], pad=sh[8], relu=relu)
        torch.cuda.synchronize()
    finally:
        ops.set_conv_bf16_tile(0)
    return y.cpu()


@functools.lru_cache(maxsize=None)
def normal_case(sh):
    """Post-ReLU normal activations, normal filters x 0.05, normal scale / shift / residual; the float64 results."""
    n, h, w, c, k, r, s, stride, pad = sh
    g = torch.Generator().manual_seed(3000 + sum(sh))
    x = torch.randn((n, h, w, c), generator=g).clamp(min=0)
    wt = torch.randn((k, r, s, c), generator=g) * 0.05
    scale, shift = torch.randn((k,), generator=g), torch.randn((k,), generator=g)
    res = torch.randn(out_shape(sh), generator=g)
    raw = conv64(x, wt, stride, pad)
    full = (raw * scale.double() + shift.double() + res.double()).clamp(min=0)
    return x, wt, scale, shift, res, raw, full


def errors(y, ref):
    d = y.double() - ref
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


@pytest.mark.gpu
@pytest.mark.parametrize("case", SMALL, ids=shape_id)
def test_small_shapes_tiles_bit_equal_and_gate(hip, case):
    """Rule tile and both forced tiles bit-equal; two runs bit-equal; largest and rms error against float64 at most 1.25 x
    the fp32 kernel's on the same operands (gate 1)."""
    sh, post = case
    x, wt, scale, shift, res, raw, full = normal_case(sh)
    args = (dev(scale), dev(shift), dev(res)) if post else (None, None, None)
    ref = full if post else raw
    xd, wd = dev(x), dev(wt)
    wp = ops.conv2d_pack_bf16x3(wd)
    ys = [run_split(xd, wp, *args, sh, post, tile) for tile in TILES]
    assert tuple(ys[0].shape) == out_shape(sh)
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    assert torch.equal(run_split(xd, wp, *args, sh, post, 0), ys[0])
    y32 = ops.conv2d_nhwc(xd, wd, *args, stride=sh[7], pad=sh[8], relu=post).cpu()
    (m3, r3), (m32, r32) = errors(ys[0], ref), errors(y32, ref)
    print("%s: split max %.3g rms %.3g, fp32 max %.3g rms %.3g (float64 reference, largest output %.3g)"
          % (shape_id(sh), m3, r3, m32, r32, float(ref.abs().max())))
    assert m3 <= GATE * m32 and r3 <= GATE * r32


@pytest.fixture
def frame_plans(hip):
    """The benchmark's tuned fp32 plan table (tile, split-K, Winograd per shape), as bench.py imports it."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(bench.__file__)), "profiles", bench.PLANS_FILE)) as f:
        ops.import_conv_plans(json.load(f))
    yield
    hip.frcnn_conv2d_clear_plans()


@pytest.mark.gpu
@pytest.mark.parametrize("sh", FRAME, ids=shape_id)
def test_frame_shapes_gate(hip, frame_plans, sh):
    """Gate 1 on the frame's four large GEMMs (the 3x3 one too, which the rule leaves to Winograd), the fp32 side under the
    benchmark's plan table, against float64 on a sample of the outputs (the first pixels of a
    1x1 layer, the first images of the 3x3 one: every output channel, the whole reduction)."""
    n, h, w, c, k, r, s, stride, pad = sh
    g = torch.Generator(device=DEV).manual_seed(sum(sh))
    x = torch.randn((n, h, w, c), generator=g, device=DEV).clamp(min=0)
    wt = torch.randn((k, r, s, c), generator=g, device=DEV) * 0.05
    y3 = ops.conv2d_nhwc_bf16x3(x, ops.conv2d_pack_bf16x3(wt), stride=stride, pad=pad)
    # the fp32 kernel this layer runs in the frame: its tuned plan (Winograd, with the pre-transformed filter, for the 3x3)
    u = ops.winograd_filter(wt) if ops.winograd_filter_wanted(n, h, w, c, k, r, s, stride, pad) else None
    assert (u is not None) == (r == 3)
    y32 = ops.conv2d_nhwc(x, wt, stride=stride, pad=pad, w_winograd=u)
    assert torch.equal(ops.conv2d_nhwc_bf16x3(x, ops.conv2d_pack_bf16x3(wt), stride=stride, pad=pad), y3)
    if r == 1:
        rows = 640
        ref = x.view(-1, c)[:rows].cpu().double() @ wt.view(k, c).cpu().double().t()
        got3, got32 = y3.view(-1, k)[:rows].cpu(), y32.view(-1, k)[:rows].cpu()
    else:
        imgs = 8
        ref = conv64(x[:imgs].cpu(), wt.cpu(), stride, pad)
        got3, got32 = y3[:imgs].cpu(), y32[:imgs].cpu()
    (m3, r3), (m32, r32) = errors(got3, ref), errors(got32, ref)
    print("%s: split max %.3g rms %.3g, fp32 max %.3g rms %.3g (float64 reference, largest output %.3g)"
          % (shape_id(sh), m3, r3, m32, r32, float(ref.abs().max())))
    assert m3 <= GATE * m32 and r3 <= GATE * r32


def _integers(sh, x_low, x_high, w_max, seed):
    """Odd integer activations with x_low <= |x| < x_high (so many significant bits), integer filter in [-w_max, w_max]."""
    n, h, w, c, k, r, s, stride, pad = sh
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(x_low // 2, x_high // 2, (n, h, w, c), generator=g) * 2 + 1
    x = (mag * (torch.randint(0, 2, (n, h, w, c), generator=g) * 2 - 1)).float()
    wt = torch.randint(-w_max, w_max + 1, (k, r, s, c), generator=g).float()
    return x, wt


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_exact_on_integer_operands(hip, tile):
    """Every partial sum below 2^24 and a filter that fits one plane: the three dropped terms are zero, every bf16 product
    and every fp32 sum is exact, so the float64 result is THE answer bit for bit."""
    # x needs two planes (12 significant bits), w one; 3x3 with padding, 18 K-steps: |sum| <= 576 * 2^12 * 2 < 2^23
    sh = SMALL[1][0]
    x, wt = _integers(sh, 2 ** 11, 2 ** 12, 2, 11)
    hi, mid, lo = split3(x)
    assert bool((mid != 0).all()) and not lo.any() and not split3(wt)[1].any()
    ref = conv64(x, wt, sh[7], sh[8])
    assert float(conv64(x.abs(), wt.abs(), sh[7], sh[8]).max()) < 2 ** 24          # every partial sum, in any order
    y = run_split(dev(x), ops.conv2d_pack_bf16x3(dev(wt)), None, None, None, sh, False, tile)
    assert torch.equal(y.double(), ref)
    # x needs all three planes (18 significant bits; half of the odd values do, the rest fit two), w in {-1, 0, 1}; stride 2,
    # three K-steps: sum |x| |w| < 2^24 is asserted
    sh = SMALL[2][0]
    x, wt = _integers(sh, 2 ** 17, 2 ** 17 + 2 ** 16, 1, 12)
    hi, mid, lo = split3(x)
    assert float((lo != 0).float().mean()) > 0.25 and bool((mid != 0).any()) and torch.equal(hi + mid + lo, x)
    ref = conv64(x, wt, sh[7], sh[8])
    assert float(conv64(x.abs(), wt.abs(), sh[7], sh[8]).max()) < 2 ** 24          # every partial sum, in any order
    y = run_split(dev(x), ops.conv2d_pack_bf16x3(dev(wt)), None, None, None, sh, False, tile)
    assert torch.equal(y.double(), ref)
    # with the shared epilogue: integer scale in {-1, .5, 1, 2}, integer shift and residual, ReLU
    sh = SMALL[3][0]
    x, wt = _integers(sh, 2 ** 9, 2 ** 10, 2, 13)
    g = torch.Generator().manual_seed(14)
    k = sh[4]
    scale = torch.tensor([-1.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (k,), generator=g)]
    shift = torch.randint(-9, 10, (k,), generator=g).float()
    res = torch.randint(-50, 51, out_shape(sh), generator=g).float()
    ref = (conv64(x, wt, sh[7], sh[8]) * scale.double() + shift.double() + res.double()).clamp(min=0)
    assert float(ref.abs().max()) < 2 ** 23
    y = run_split(dev(x), ops.conv2d_pack_bf16x3(dev(wt)), dev(scale), dev(shift), dev(res), sh, True, tile)
    assert torch.equal(y.double(), ref)


SPECIAL_BITS = (0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0x3F800080, 0x3F800180, 0x3F80807F, 0x3F808081,
                0x3F818080, 0x3FFFFFFF, 0x3F7FFFFF, 0x4B7FFFFF, 0x7E7FFFFF, 0x00000000, 0x80000000, 0x3F800000, 0x40490FDB)


@pytest.mark.gpu
def test_pack_splits_as_the_host_does(hip):
    """frcnn_conv2d_pack_bf16x3 against ``split3``: the device conversion rounds to nearest even on the remainders as on the
    values (ties in the first and in the second remainder among the patterns), plane by plane, and the planes add up."""
    g = torch.Generator().manual_seed(5)
    special = torch.tensor(SPECIAL_BITS, dtype=torch.int64).to(torch.int32).view(torch.float32)
    w = torch.cat([special, torch.randn(4096 - len(SPECIAL_BITS), generator=g) * 0.05]).view(4, 1, 1, 1024)
    got = ops.conv2d_pack_bf16x3(dev(w)).cpu()
    assert got.shape == (3, 4, 1, 1, 1024) and got.dtype == torch.int16
    planes = [(p.to(torch.int32) << 16).view(torch.float32) for p in got]
    for have, want in zip(planes, split3(w)):
        assert torch.equal(have.view(torch.int32), want.view(torch.int32))
    assert torch.equal((planes[0] + planes[1]) + planes[2], w)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_activation_planes_add_up_for_every_pattern(hip, tile):
    """The in-kernel split of the activations (vector conversions, not the packer's scalar ones): through an identity filter
    an output is hi + mid + lo of one activation and nothing else, so it must be that activation bit for bit - for the tie
    patterns of SPECIAL_BITS (ties in the value, in the first and in the second remainder), for values with all 24 bits set
    and for random ones.  No single plane shows in an output - any three planes that add up exactly give the same six
    products, up to the dropped 2^-26 - so what is pinned is what the arithmetic needs: no plane loses a bit."""
    g = torch.Generator().manual_seed(6)
    special = torch.tensor(SPECIAL_BITS, dtype=torch.int64).to(torch.int32).view(torch.float32)
    x = torch.cat([special, torch.randn(3 * 5 * 64 - len(SPECIAL_BITS), generator=g) * 3]).view(3, 5, 1, 64)
    eye = torch.eye(64).view(64, 1, 1, 64).contiguous()
    y = run_split(dev(x), ops.conv2d_pack_bf16x3(dev(eye)), None, None, None, (3, 5, 1, 64, 64, 1, 1, 1, 0), False, tile)
    assert torch.equal(y, x)


@pytest.mark.gpu
def test_operand_range(hip):
    """Finite operands up to about 2^120 come out as from fp32; an infinite activation gives NaN where fp32 gives infinity
    (its remainder is inf - inf) - the documented limit of the split path."""
    sh = (1, 4, 4, 32, 8, 1, 1, 1, 0)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (1, 4, 4, 32), generator=g).float() * 2.0 ** 110
    wt = torch.randint(-2, 3, (8, 1, 1, 32), generator=g).float()
    ref = conv64(x, wt, 1, 0)
    y = run_split(dev(x), ops.conv2d_pack_bf16x3(dev(wt)), None, None, None, sh, False, 0)
    assert torch.equal(y.double(), ref)
    x[0, 1, 2, 5] = float("inf")
    wt[:, 0, 0, 5] = 1.0
    ref = conv64(x, wt, 1, 0)
    y = run_split(dev(x), ops.conv2d_pack_bf16x3(dev(wt)), None, None, None, sh, False, 0)
    y32 = ops.conv2d_nhwc(dev(x), dev(wt)).cpu()
    assert bool(torch.isinf(y32[0, 1, 2]).all()) and bool(torch.isnan(y[0, 1, 2]).all())
    keep = torch.ones(4, 4, dtype=torch.bool)
    keep[1, 2] = False
    assert torch.equal(y[0][keep].double(), ref[0][keep])          # the other pixels do not see it
    # near the smallest normals: a remainder below 2^-126 may flush, so an operand of 2^-120 .. 2^-119 with 24 significant
    # bits arrives as the sum of its planes with every subnormal plane either kept or dropped (identity filter, one product)
    g = torch.Generator().manual_seed(4)
    x = ((1 + torch.rand((1, 4, 4, 32), generator=g)) * 2.0 ** -120).float()
    eye = torch.eye(32).view(32, 1, 1, 32).contiguous()
    y = run_split(dev(x), ops.conv2d_pack_bf16x3(dev(eye)), None, None, None, (1, 4, 4, 32, 32, 1, 1, 1, 0), False, 0)
    hi, mid, lo = (p.double() for p in split3(x))
    assert bool((mid.abs() < 2.0 ** -126).all()) and bool((mid != 0).any())
    allowed = [hi + a * mid + b * lo for a in (0, 1) for b in (0, 1)]
    assert bool(torch.stack([y.double() == v for v in allowed]).any(0).all())
    print("operands near 2^-120: %d of %d outputs equal the full sum, %d the leading plane alone"
          % (int((y.double() == allowed[3]).sum()), y.numel(), int((y.double() == allowed[0]).sum())))


# ---- GPU: through the net -----------------------------------------------------------------------------------------------------
def _image_net(seed=5):
    from oracle import frcnn_oracle as O
    from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
    C.reset_cfg()
    C.cfg.NET_TYPE = "image"
    oracle = O.ImageNetOracle(num_classes=2)
    sd = O.seeded_state_dict(oracle, seed, bn_mode="tame")
    net = imagenet(num_layers=101)
    net.create_architecture(2, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
    net.load_state_dict(sd, strict=True)
    net.eval()
    net._device = DEV
    net.to(DEV)
    return net


def _frame_outputs(net, data, info):
    with torch.no_grad():
        net.forward(data, info, None, None, mode="TEST")
    torch.cuda.synchronize()
    p = net._predictions
    n = int(p["rois_count"].item())
    return {"net_conv": net._act_summaries["conv"].clone(), "n": n, "rois": p["rois"][:n].clone(),
            "cls_prob": p["cls_prob"][:n].clone(), "bbox_pred": p["bbox_pred"][:n].clone()}


@pytest.mark.gpu
def test_through_the_net(hip):
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FramePool
    from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device
    net = _image_net()
    h, w = 192, 320                                  # the smallest frame of the image detector's parity tests
    rng = np.random.default_rng(7)
    data = torch.from_numpy((rng.standard_normal((1, h, w, 3)) * 50).astype(np.float32)).to(DEV)
    info = np.array([0, w, 0, h, 0, 0, 1.0], np.float32)
    saved_profile = ops.PROFILE
    try:
        # ---- switch off is today's fp32 path; switch on moves exactly the calls the rule selects
        C.cfg.TEST.CONV_SPLIT_BF16 = False
        ops.PROFILE = []
        off = _frame_outputs(net, data, info)
        convs = list(ops.PROFILE)
        assert not any(p.get("split_bf16") or p.get("bf16") for p in convs)
        C.cfg.TEST.CONV_SPLIT_BF16 = True
        ops.PROFILE = []
        on = _frame_outputs(net, data, info)
        taken = list(ops.PROFILE)
        ops.PROFILE = saved_profile
        geom = lambda p: (p["n"], p["h"], p["w"], p["c"], p["k"], p["r"], p["s"], p["stride"], p["pad"])
        assert [geom(p) for p in taken] == [geom(p) for p in convs]
        assert all(bool(p.get("split_bf16")) == (p["c"] % 32 == 0 and ops.conv_split_bf16_wanted(*geom(p))) for p in taken)
        n_split = sum(1 for p in taken if p.get("split_bf16"))
        print("%d of %d convolutions of the frame take the split kernel" % (n_split, len(taken)))
        assert 0 < n_split < len(taken) and not any(p.get("bf16") for p in taken)
        # the backbone holds no selected layer on this frame (a 12 x 20 map: every GEMM is below the rule), layer4 on the
        # 300 RoI rows does: net_conv does not move at all, the heads do
        assert all(p["n"] > 1 for p in taken if p.get("split_bf16"))
        rel = float((on["net_conv"] - off["net_conv"]).double().norm() / off["net_conv"].double().norm())
        # same injected RPN output on both sides (as tests/test_conv_bf16.py): row i is RoI i
        cls, box = bench.structured_rpn(7, h=off["net_conv"].shape[1], w=off["net_conv"].shape[2])
        net._rpn_override = bench.fuse_rpn(cls, box).to(DEV)
        try:
            C.cfg.TEST.CONV_SPLIT_BF16 = False
            heads32 = _frame_outputs(net, data, info)
            C.cfg.TEST.CONV_SPLIT_BF16 = True
            heads3 = _frame_outputs(net, data, info)
        finally:
            net._rpn_override = None
        assert heads32["n"] == heads3["n"] > 0 and torch.equal(heads32["rois"], heads3["rois"])
        gap_cls = float((heads3["cls_prob"] - heads32["cls_prob"]).abs().max())
        gap_box = float((heads3["bbox_pred"] - heads32["bbox_pred"]).abs().max())
        print("net_conv relative L2 gap %.4g; %d RoIs: cls_prob max-abs gap %.4g (recorded %.4g), bbox_pred "
              "max-abs gap %.4g (recorded %.4g), |bbox_pred| max %.4g"
              % (rel, heads32["n"], gap_cls, CLS_PROB_MAX_ABS, gap_box, BBOX_PRED_MAX_ABS,
                 float(heads32["bbox_pred"].abs().max())))
        assert rel == 0.0
        assert gap_cls <= 4 * CLS_PROB_MAX_ABS
        assert gap_box <= 4 * BBOX_PRED_MAX_ABS
        # ---- a captured frame replays bit-equal to the eager frame; toggling the switch captures again
        thresh, max_dets = 0.05, 100
        pool = FramePool(net, streams=1, capture_after=1, autotune=False)
        results = {}
        for switch in (True, False, True):
            C.cfg.TEST.CONV_SPLIT_BF16 = switch
            with torch.no_grad():
                dets, counts = detect_frame_device(net, data, info, thresh, max_dets, max_dets)
            torch.cuda.synchronize()
            runner = pool.runner((1, h, w, 3), info, thresh, max_dets)
            assert runner is not None
            for _ in range(2):
                g_d, g_c = runner.run(data)
                torch.cuda.synchronize()
                assert torch.equal(g_c, counts) and torch.equal(g_d, dets)
            assert results.get(switch, runner) is runner          # back to a setting: its captured frame is found again
            results[switch] = runner
            assert pool.stats["captures"] == (1 if not results.get(False) else 2)
        assert results[True] is not results[False] and len(pool.runners) == 2
    finally:
        ops.PROFILE = saved_profile
        H.set_net_mode(None)
        C.reset_cfg()
