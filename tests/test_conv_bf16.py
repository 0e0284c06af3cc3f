"""bf16-operand forward convolutions (cfg.TEST.CONV_BF16): ``frcnn_conv2d_pack_bf16`` / ``frcnn_conv2d_fwd_bf16``, the
``ops`` wrappers, ``hip_modules.conv_bf16_eligible`` / ``conv_forward`` and the switch's way through the image detector and
the captured frame.

The math under test is ``y = act((sum bf16(x) * bf16(w)) * scale + shift + residual)`` with fp32 accumulation.  The
yardstick is always a float64 convolution on the host (``conv64``) of operands rounded to bf16 BY TORCH ON THE CPU - never
the device's rounding and never the fp32 kernels.

Every kernel test runs every shape of ``SHAPES`` under both forced tiles (64x64, 128x128) and with and without the epilogue
operands.  Host references are computed once per shape and shared (``exact_case`` / ``normal_case``), read-only.

Through the net (``test_through_the_net``) no bound can be derived for 100 layers of 2^-9 operand rounding: the gaps to
the fp32 path on the same frame and weights were measured on an MI355X (profiles/conv_bf16.md) and are held to 4x the
recorded values, and must be above zero.
"""
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
FRCNN_ERR_ARG = -1           # include/frcnn_hip.h
# (n, h, w, c, k, r, s, stride, pad): one pixel; K below a tile, K not a multiple of 4 / 32; M = 35, 126 (an image boundary
# inside a tile), 272; odd maps under stride 2; 144 K-steps
SHAPES = [(1, 1, 1, 32, 4, 1, 1, 1, 0), (1, 5, 7, 32, 18, 1, 1, 1, 0), (1, 5, 7, 32, 36, 1, 1, 1, 0),
          (2, 9, 7, 64, 132, 3, 3, 1, 1), (1, 13, 11, 96, 64, 3, 3, 2, 1), (1, 8, 8, 128, 256, 1, 1, 2, 0),
          (1, 17, 16, 32, 68, 3, 3, 1, 1), (1, 12, 20, 256, 128, 1, 1, 1, 0), (1, 6, 6, 512, 32, 3, 3, 1, 1)]
SHORT_K = [sh for sh in SHAPES if sh[3] * sh[5] * sh[6] <= 1200]          # the fp32-accumulation bound's range
TILES = (1, 2)
# measured on an MI355X, recorded in profiles/conv_bf16.md (ResNet-101 image detector, 192x320 frame, seed 5 / frame 7)
NET_CONV_REL_L2, CLS_PROB_MAX_ABS, BBOX_PRED_MAX_ABS = 5.287e-3, 6.688e-5, 2.538e-2


def shape_id(sh):
    return "n%d_%dx%d_c%d_k%d_%dx%d_s%d_p%d" % sh


def conv64(x_nhwc, w_krsc, stride, pad):
    """float64 convolution on the host: NHWC input, KRSC filter -> NHWC output."""
    y = F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w_krsc.double().permute(0, 3, 1, 2), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


def out_shape(sh):
    n, h, w, c, k, r, s, stride, pad = sh
    return n, (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1, k


def bf16_round(t):
    """fp32 -> bf16 -> fp32 by torch on the CPU (round to nearest even)."""
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def exact_case(sh):
    """Integer operands: x in [-8, 8] with the extremes on the map border, w in [-4, 4], scale in {-1, .5, 1, 2}, integer
    shift and residual.  Products and partial sums stay below 2^24 (4608 * 32), bf16 holds the operands exactly: the
    float64 result cast to fp32 is THE answer in any summation order."""
    n, h, w, c, k, r, s, stride, pad = sh
    g = torch.Generator().manual_seed(1000 + sum(sh))
    x = torch.randint(-6, 7, (n, h, w, c), generator=g).float()
    border = torch.zeros(h, w, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    sign = torch.randint(0, 2, (n, h, w, c), generator=g).float() * 2 - 1
    x = torch.where(border[None, :, :, None], 8 * sign, x)
    wt = torch.randint(-4, 5, (k, r, s, c), generator=g).float()
    scale = torch.tensor([-1.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (k,), generator=g)]
    shift = torch.randint(-9, 10, (k,), generator=g).float()
    res = torch.randint(-50, 51, out_shape(sh), generator=g).float()
    acc = conv64(x, wt, stride, pad)
    assert float(acc.abs().max()) < 2 ** 24
    full = acc * scale.double() + shift.double() + res.double()
    want = {(False, False): acc.float(), (False, True): acc.clamp(min=0).float(),
            (True, False): full.float(), (True, True): full.clamp(min=0).float()}
    assert all(torch.equal(v.double(), ref) for v, ref in ((want[(False, False)], acc), (want[(True, False)], full)))
    return x, wt, scale, shift, res, want


@functools.lru_cache(maxsize=None)
def normal_case(sh):
    """Random normal operands; r = float64 convolution of the HOST-rounded operands, S = the same of their absolute values."""
    n, h, w, c, k, r, s, stride, pad = sh
    g = torch.Generator().manual_seed(2000 + sum(sh))
    x = torch.randn((n, h, w, c), generator=g)
    wt = torch.randn((k, r, s, c), generator=g) * 0.1
    scale = torch.randn((k,), generator=g)
    shift = torch.randn((k,), generator=g)
    res = torch.randn(out_shape(sh), generator=g)
    xr, wr = bf16_round(x), bf16_round(wt)
    ref = conv64(xr, wr, stride, pad)
    mag = conv64(xr.abs(), wr.abs(), stride, pad)
    return x, wt, scale, shift, res, xr, wr, ref, mag


def run_bf16(x, w_packed, scale, shift, res, sh, relu, tile):
    stride, pad = sh[7], sh[8]
    ops.set_conv_bf16_tile(tile)
    try:
        y = ops.conv2d_nhwc_bf16(x, w_packed, scale, shift, res, stride=stride, pad=pad, relu=relu)
        torch.cuda.synchronize()
    finally:
        ops.set_conv_bf16_tile(0)
    return y.cpu()


def dev(t):
    return None if t is None else t.to(DEV)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_switch_is_off_by_default():
    C.reset_cfg()
    assert C.cfg.TEST.CONV_BF16 is False


@pytest.mark.parametrize("c,want", [(3, False), (4, False), (20, False), (32, True), (64, True), (2048, True)])
def test_eligible_truth_table(c, want):
    for k in (1, 18, 36, 256):
        for r, stride, pad in ((1, 1, 0), (3, 1, 1), (3, 2, 1), (1, 2, 0), (7, 2, 3)):
            assert H.conv_bf16_eligible(c, k, r, r, stride, pad, False) is want
            assert H.conv_bf16_eligible(c, k, r, r, stride, pad, True) is False         # strided output: never


def test_wrappers_reject_bad_arguments_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_hip, "load", no_library)
    x = torch.zeros(1, 4, 4, 32)
    w16 = torch.zeros(8, 1, 1, 32, dtype=torch.int16)
    with pytest.raises(_hip.HipError):
        ops.conv2d_pack_bf16(torch.zeros(8, 1, 1, 32))                                 # CPU tensor
    with pytest.raises(_hip.HipError):
        ops.conv2d_pack_bf16(torch.zeros(8, 1, 1, 32, dtype=torch.float64))
    with pytest.raises(_hip.HipError):
        ops.conv2d_nhwc_bf16(x, w16)                                                    # CPU tensors
    with pytest.raises(_hip.HipError):
        ops.conv2d_nhwc_bf16(x.double(), w16)

    class OnDevice(torch.Tensor):       # a host tensor that claims to be on the device: reaches the shape / dtype checks
        is_cuda = True

    def fake(t):
        return t.as_subclass(OnDevice)
    good_x, good_w = fake(x), fake(w16)
    bad = [(fake(torch.zeros(1, 4, 4, 48)), fake(torch.zeros(8, 1, 1, 48, dtype=torch.int16)), {}),      # C % 32 != 0
           (fake(torch.zeros(1, 4, 4, 64)), good_w, {}),                                                  # channel mismatch
           (good_x, fake(torch.zeros(8, 1, 1, 32)), {}),                                                  # fp32 filter
           (good_x, fake(torch.zeros(8, 32, dtype=torch.int16)), {}),                                     # not 4-D
           (fake(torch.zeros(4, 4, 32)), good_w, {}),                                                     # x not 4-D
           (good_x, fake(torch.zeros(8, 5, 5, 32, dtype=torch.int16)), {}),                               # filter larger than the map
           (good_x, good_w, {"stride": 0}), (good_x, good_w, {"pad": -1}),
           (good_x, good_w, {"scale": fake(torch.zeros(7))}), (good_x, good_w, {"shift": fake(torch.zeros(9))}),
           (good_x, good_w, {"shift": fake(torch.zeros(8, dtype=torch.float64))}),
           (good_x, good_w, {"residual": fake(torch.zeros(1, 4, 4, 4))}),
           (good_x, good_w, {"out": fake(torch.zeros(1, 4, 4, 4))}),
           (fake(torch.zeros(1, 4, 32, 4).permute(0, 1, 3, 2)), good_w, {})]                              # not contiguous
    for bx, bw, kw in bad:
        with pytest.raises(_hip.HipError):
            ops.conv2d_nhwc_bf16(bx, bw, **kw)
    with pytest.raises(_hip.HipError):
        ops.conv2d_pack_bf16(fake(torch.zeros(8, 32)))


def test_frame_graph_key_carries_the_switch():
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import cfg_fingerprint
    C.reset_cfg()
    net = torch.nn.Sequential(torch.nn.Conv2d(4, 4, 1))
    try:
        off = cfg_fingerprint(net)
        C.cfg.TEST.CONV_BF16 = True
        on = cfg_fingerprint(net)
        C.cfg.TEST.CONV_BF16 = False
        assert cfg_fingerprint(net) == off and on != off
        assert sum(a != b for a, b in zip(on, off)) == 1
    finally:
        C.reset_cfg()


def test_dispatch_takes_bf16_only_in_test_mode_without_gradient(monkeypatch):
    """``conv_bf16_wanted`` on host tensors: switch, net mode, eligibility, gradient."""
    C.reset_cfg()
    x, w = torch.zeros(1, 4, 4, 32), torch.zeros(8, 3, 3, 32)
    try:
        for switch in (False, True):
            for mode in (None, "TRAIN", "TEST"):
                C.cfg.TEST.CONV_BF16 = switch
                H.set_net_mode(mode)
                with torch.no_grad():
                    assert H.conv_bf16_wanted(x, w, 1, 1) is (switch and mode == "TEST")
                    assert H.conv_bf16_wanted(torch.zeros(1, 4, 4, 20), torch.zeros(8, 3, 3, 20), 1, 1) is False
                assert H.conv_bf16_wanted(x.clone().requires_grad_(True), w, 1, 1) is False
    finally:
        H.set_net_mode(None)
        C.reset_cfg()


# ---- GPU: the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sh", SHAPES, ids=shape_id)
def test_exact_on_integer_operands(hip, sh):
    x, wt, scale, shift, res, want = exact_case(sh)
    xd, wp = dev(x), ops.conv2d_pack_bf16(dev(wt))
    for tile in TILES:
        for full in (False, True):
            for relu in (False, True):
                got = run_bf16(xd, wp, dev(scale) if full else None, dev(shift) if full else None, dev(res) if full else None,
                               sh, relu, tile)
                ref = want[(full, relu)]
                bad = int((got != ref).sum())
                print("%s tile %d full %d relu %d: %d of %d differ" % (shape_id(sh), tile, full, relu, bad, ref.numel()))
                assert got.shape == ref.shape and bad == 0
    # scale / shift / residual one at a time (each operand's own null branch)
    acc = conv64(x, wt, sh[7], sh[8])
    for tile in TILES:
        assert torch.equal(run_bf16(xd, wp, dev(scale), None, None, sh, False, tile), (acc * scale.double()).float())
        assert torch.equal(run_bf16(xd, wp, None, dev(shift), None, sh, False, tile), (acc + shift.double()).float())
        assert torch.equal(run_bf16(xd, wp, None, None, dev(res), sh, True, tile), (acc + res.double()).clamp(min=0).float())


def f32_from_bits(*bits):
    return torch.tensor(np.array(bits, dtype=np.uint32).view(np.float32))


# exact ties with an even (0x3F80 stays) and an odd (0x3F81 -> 0x3F82) kept mantissa, just below / above a tie, a value
# that rounds into the next exponent (0x3FFF8000 -> 0x4000) and into inf, the largest bf16, denormal-free small values, +-0, +-inf
SPECIAL_BITS = (0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x3FFF8000, 0x3FFFFFFF, 0x7F7F8000,
                0x7F7F7FFF, 0x7F7F0000, 0x00800000, 0x00808000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000,
                0x40490FDB, 0xC0490FDB)


@pytest.mark.gpu
def test_pack_rounds_to_nearest_even(hip):
    special = f32_from_bits(*SPECIAL_BITS)
    g = torch.Generator().manual_seed(7)
    w = torch.cat((special, torch.randn(4 * 3 * 3 * 32 - special.numel(), generator=g) * 3)).view(4, 3, 3, 32)
    want = w.to(torch.bfloat16).view(torch.int16)
    assert want.view(-1)[0].item() == 0x3F80 and want.view(-1)[1].item() == 0x3F82 and want.view(-1)[6].item() == 0x4000
    got = ops.conv2d_pack_bf16(dev(w))
    torch.cuda.synchronize()
    assert got.dtype == torch.int16 and got.shape == w.shape and torch.equal(got.cpu(), want)
    assert hip.frcnn_conv2d_pack_bf16_bytes(4, 3, 3, 32) == w.numel() * 2 and hip.frcnn_conv2d_pack_bf16_bytes(4, 0, 3, 32) == 0
    # NaN stays NaN (quiet or signalling, either sign; the payload is not pinned)
    nan = f32_from_bits(0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F80FFFF, 0xFF800001).repeat(6)[:32].reshape(1, 1, 1, 32)
    assert bool(torch.isnan(nan).all())
    packed = ops.conv2d_pack_bf16(dev(nan)).cpu()
    assert bool(torch.isnan(packed.view(torch.bfloat16).float()).all())


@pytest.mark.gpu
@pytest.mark.parametrize("sh", SHAPES, ids=shape_id)
def test_activations_and_filter_are_rounded_as_on_the_host(hip, sh):
    """fwd_bf16(x, pack(w)) is bit-equal to the same call on operands rounded to bf16 on the host first; the activations
    carry exact ties too."""
    x, wt, scale, shift, res, xr, wr, _, _ = normal_case(sh)
    x = x.clone()
    flat = x.view(-1)
    ties = f32_from_bits(*[b for b in SPECIAL_BITS if (b & 0x7F800000) != 0x7F800000 and b != 0x7F7F8000])
    flat[:min(ties.numel(), flat.numel())] = ties[:flat.numel()]
    xr = bf16_round(x)
    assert not torch.equal(x, xr) and not torch.equal(wt, wr)
    for tile in TILES:
        a = run_bf16(dev(x), ops.conv2d_pack_bf16(dev(wt)), dev(scale), dev(shift), dev(res), sh, True, tile)
        b = run_bf16(dev(xr), ops.conv2d_pack_bf16(dev(wr)), dev(scale), dev(shift), dev(res), sh, True, tile)
        assert torch.equal(a, b)
        a = run_bf16(dev(x), ops.conv2d_pack_bf16(dev(wt)), None, None, None, sh, False, tile)
        b = run_bf16(dev(xr), ops.conv2d_pack_bf16(dev(wr)), None, None, None, sh, False, tile)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.gpu
@pytest.mark.parametrize("sh", SHORT_K, ids=shape_id)
def test_accumulation_is_fp32(hip, sh):
    """|y - (r scale + shift + res)| <= (R S C + 8) 2^-23 (S |scale| + |shift| + |res|): one fp32 ulp per accumulation in any
    order, rounded or truncated; a dropped term is about ten times larger up to R S C = 1200."""
    x, wt, scale, shift, res, xr, wr, ref, mag = normal_case(sh)
    terms = sh[3] * sh[5] * sh[6]
    wp = ops.conv2d_pack_bf16(dev(wt))
    for tile in TILES:
        for full in (False, True):
            for relu in (False, True):
                got = run_bf16(dev(x), wp, dev(scale) if full else None, dev(shift) if full else None, dev(res) if full else None,
                               sh, relu, tile).double()
                if full:
                    want = ref * scale.double() + shift.double() + res.double()
                    room = mag * scale.double().abs() + shift.double().abs() + res.double().abs()
                else:
                    want, room = ref, mag
                if relu:
                    want = want.clamp(min=0)              # 1-Lipschitz: the bound carries over
                tol = (terms + 8) * 2.0 ** -23 * room
                worst = float(((got - want).abs() / tol).max())
                print("%s tile %d full %d relu %d: worst error / tolerance %.3f" % (shape_id(sh), tile, full, relu, worst))
                assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("sh", SHAPES, ids=shape_id)
def test_tiles_are_bit_identical(hip, sh):
    x, wt, scale, shift, res = normal_case(sh)[:5]
    wp = ops.conv2d_pack_bf16(dev(wt))
    for full in (False, True):
        for relu in (False, True):
            args = (dev(x), wp, dev(scale) if full else None, dev(shift) if full else None, dev(res) if full else None, sh, relu)
            small, large, auto = run_bf16(*args, 1), run_bf16(*args, 2), run_bf16(*args, 0)
            assert torch.equal(small, large) and torch.equal(small, auto)


# ---- GPU: nothing else moved ------------------------------------------------------------------------------------------------
def _conv_module(c, k, r, stride, pad, seed):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(c, k, r, stride=stride, padding=pad, bias=False)
    bn = torch.nn.BatchNorm2d(k)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 1.5)
    conv.eval(), bn.eval()
    return conv.to(DEV), bn.to(DEV)


@pytest.mark.gpu
def test_nothing_else_moved(hip):
    C.reset_cfg()
    sig = hip.frcnn_settings_signature()
    try:
        H.set_net_mode("TEST")
        with torch.no_grad():
            for c in (64, 20):
                conv, bn = _conv_module(c, 24, 3, 1, 1, seed=c)
                g = torch.Generator().manual_seed(c)
                x = torch.randn((1, 9, 11, c), generator=g).to(DEV)
                res = torch.randn((1, 9, 11, 24), generator=g).to(DEV)
                w, scale, shift = H.prepared_conv(conv, bn)
                xp = ops.pad_channels(x, w.shape[-1]) if x.shape[-1] != w.shape[-1] else x
                ref = ops.conv2d_nhwc(xp, w, scale, shift, res, stride=1, pad=1, relu=True)
                C.cfg.TEST.CONV_BF16 = False
                off = H.conv_bn_act(x, conv, bn, relu=True, residual=res)
                assert torch.equal(off, ref) and "_frcnn_bf16" not in conv.__dict__
                C.cfg.TEST.CONV_BF16 = True
                on = H.conv_bn_act(x, conv, bn, relu=True, residual=res)
                if c % 32:
                    assert torch.equal(on, ref) and "_frcnn_bf16" not in conv.__dict__       # C % 32 != 0: the fp32 path
                else:
                    want = ops.conv2d_nhwc_bf16(x, ops.conv2d_pack_bf16(w), scale, shift, res, stride=1, pad=1, relu=True)
                    assert torch.equal(on, want) and not torch.equal(on, ref) and "_frcnn_bf16" in conv.__dict__
                    H.set_net_mode("TRAIN")                # a training forward ignores the switch
                    assert torch.equal(H.conv_bn_act(x, conv, bn, relu=True, residual=res), ref)
                    H.set_net_mode("TEST")
        # the C entry point refuses C % 32 != 0 with a message
        x = torch.zeros(1, 4, 4, 48, device=DEV)
        w16 = torch.zeros(8, 1, 1, 48, dtype=torch.int16, device=DEV)
        y = torch.zeros(1, 4, 4, 8, device=DEV)
        rc = hip.frcnn_conv2d_fwd_bf16(x.data_ptr(), w16.data_ptr(), None, None, None, y.data_ptr(), 1, 4, 4, 48, 8, 1, 1, 1, 0, 0,
                                       None)
        assert rc == FRCNN_ERR_ARG and b"c%32==0" in hip.frcnn_last_error()
        rc = hip.frcnn_conv2d_fwd_bf16(x.data_ptr(), w16.data_ptr(), None, None, None, y.data_ptr(), 1, 4, 4, 32, 8, 5, 5, 1, 0, 0,
                                       None)
        assert rc == FRCNN_ERR_ARG and b"bad shape" in hip.frcnn_last_error()
        assert hip.frcnn_conv2d_bf16_set_tile(3) == FRCNN_ERR_ARG and hip.frcnn_conv2d_bf16_set_tile(-1) == FRCNN_ERR_ARG
        # the settings signature: today's value at mode 0, another one under a forced tile
        assert hip.frcnn_settings_signature() == sig
        ops.set_conv_bf16_tile(1)
        one = hip.frcnn_settings_signature()
        ops.set_conv_bf16_tile(2)
        two = hip.frcnn_settings_signature()
        ops.set_conv_bf16_tile(0)
        assert one != sig and two != sig and one != two and hip.frcnn_settings_signature() == sig
    finally:
        ops.set_conv_bf16_tile(0)
        H.set_net_mode(None)
        C.reset_cfg()


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
def test_through_the_net(hip, monkeypatch):
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
    net = _image_net()
    h, w = 192, 320                                  # the smallest frame of the image detector's parity tests
    rng = np.random.default_rng(7)
    data = torch.from_numpy((rng.standard_normal((1, h, w, 3)) * 50).astype(np.float32)).to(DEV)
    info = np.array([0, w, 0, h, 0, 0, 1.0], np.float32)
    saved_profile = ops.PROFILE
    real_bf16 = ops.conv2d_nhwc_bf16
    calls = []

    def counting(x, w_bf16, *a, **kw):
        calls.append((tuple(x.shape), tuple(w_bf16.shape)))
        return real_bf16(x, w_bf16, *a, **kw)
    try:
        # ---- switch off: the frame's convolutions, and the fp32 yardstick
        ops.PROFILE = []
        fp32 = _frame_outputs(net, data, info)
        convs = list(ops.PROFILE)
        assert not any(p.get("bf16") for p in convs)
        eligible = [p for p in convs if p["c"] % 32 == 0]
        assert len(convs) > 100 and 0 < len(eligible) < len(convs)
        # ---- switch on
        C.cfg.TEST.CONV_BF16 = True
        monkeypatch.setattr(ops, "conv2d_nhwc_bf16", counting)
        ops.PROFILE = []
        bf16 = _frame_outputs(net, data, info)
        on = list(ops.PROFILE)
        assert len(calls) == len(eligible) == sum(1 for p in on if p.get("bf16"))
        assert [(p["c"], p["k"], p["r"], p["stride"]) for p in on] == [(p["c"], p["k"], p["r"], p["stride"]) for p in convs]
        stem = on[0]
        assert stem["r"] == 7 and stem["c"] == 4 and not stem.get("bf16")                 # the stem conv stays fp32
        assert all(bool(p.get("bf16")) == (p["c"] % 32 == 0) for p in on)
        ops.PROFILE = saved_profile
        # ---- distance to the fp32 path (same frame, same weights)
        rel = float((bf16["net_conv"] - fp32["net_conv"]).double().norm() / fp32["net_conv"].double().norm())
        print("net_conv relative L2 gap %.4g (recorded %.4g)" % (rel, NET_CONV_REL_L2))
        assert 0.0 < rel <= 4 * NET_CONV_REL_L2
        # The heads' rows are comparable only on the same proposals, and the two paths rank a random-weight RPN's near-equal
        # scores differently: both paths get the same injected RPN output (the evaluation hook of the parity tests and of
        # bench.py's structured frames), so that row i is RoI i on both sides.  Backbone, layer4 and heads are each path's own.
        cls, box = bench.structured_rpn(7, h=fp32["net_conv"].shape[1], w=fp32["net_conv"].shape[2])
        net._rpn_override = bench.fuse_rpn(cls, box).to(DEV)
        try:
            C.cfg.TEST.CONV_BF16 = False
            heads32 = _frame_outputs(net, data, info)
            C.cfg.TEST.CONV_BF16 = True
            heads16 = _frame_outputs(net, data, info)
        finally:
            net._rpn_override = None
        assert heads32["n"] == heads16["n"] > 0 and torch.equal(heads32["rois"], heads16["rois"])
        gap_cls = float((heads16["cls_prob"] - heads32["cls_prob"]).abs().max())
        gap_box = float((heads16["bbox_pred"] - heads32["bbox_pred"]).abs().max())
        print("%d RoIs: cls_prob max-abs gap %.4g (recorded %.4g), bbox_pred max-abs gap %.4g (recorded %.4g), |bbox_pred| max %.4g"
              % (heads32["n"], gap_cls, CLS_PROB_MAX_ABS, gap_box, BBOX_PRED_MAX_ABS, float(heads32["bbox_pred"].abs().max())))
        assert 0.0 < gap_cls <= 4 * CLS_PROB_MAX_ABS
        assert 0.0 < gap_box <= 4 * BBOX_PRED_MAX_ABS
        # ---- a captured frame equals the eager frame
        from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device
        thresh, max_dets = 0.05, 100
        with torch.no_grad():
            dets, counts = detect_frame_device(net, data, info, thresh, max_dets, max_dets)
        torch.cuda.synchronize()
        n_eager = len(calls)
        runner = FrameRunner(net, h, w, 3, info, thresh, max_dets, autotune=False)
        for _ in range(2):
            g_d, g_c = runner.run(data)
            torch.cuda.synchronize()
            assert torch.equal(g_c, counts) and torch.equal(g_d, dets)
        assert len(calls) > n_eager                   # the runner's warm-up and captured frames took the bf16 entry too
        # ---- an in-place weight change reaches the packed filter through refresh_derived_weights
        conv = net.resnet.layer2[0].conv1
        packed = conv.__dict__["_frcnn_bf16"][1][0]
        before, address = packed.clone(), packed.data_ptr()
        with torch.no_grad():
            conv.weight.mul_(-1.5)
            H.refresh_derived_weights(net)
        torch.cuda.synchronize()
        packed = conv.__dict__["_frcnn_bf16"][1][0]
        want = ops.conv2d_pack_bf16(H.prepared_conv(conv, net.resnet.layer2[0].bn1)[0])
        assert packed.data_ptr() == address and torch.equal(packed, want) and not torch.equal(packed, before)
        with torch.no_grad():
            dets2, counts2 = detect_frame_device(net, data, info, thresh, max_dets, max_dets)
        g_d, g_c = runner.run(data)
        torch.cuda.synchronize()
        assert torch.equal(g_c, counts2) and torch.equal(g_d, dets2)          # the replayed graph reads the re-packed filter
        moved = _frame_outputs(net, data, info)
        assert not torch.equal(moved["net_conv"], bf16["net_conv"])          # the output follows the new weights
    finally:
        ops.PROFILE = saved_profile
        H.set_net_mode(None)
        C.reset_cfg()
