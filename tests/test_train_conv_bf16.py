"""cfg.TRAIN.CONV_BF16: bf16-operand convolutions in the training step (forward, data gradient, filter gradient of the eligible
convolutions of the Bottleneck and conv_bn_act_train nodes; nets/hip_modules.conv_bf16_train_eligible).

The small net (tests/bf16_train_restatement.small_net, on a 12 x 16 map, BATCH frames): conv0 3x3 8 -> 64 with a bias (C = 8: NOT
eligible), conv0b 1x1 64 -> 64 with a bias, Bottleneck a (64 -> 32 -> 128, stride-2 3x3, stride-2 1x1 projection) and
Bottleneck b (128 -> 32 -> 128), BatchNorms frozen with non-trivial statistics.  loss = sum(output * g), g a fixed cotangent.

Against the restatement.  Per tensor (the output and every parameter gradient) the relative error
||device - float64||_2 / ||float64||_2 is compared with the same quantity r32 of the restatement run in float32 on the host -
another fp32 evaluation of the same function.  Bound: BOUND_FACTOR = 8 times r32, the factor of tests/test_vgg16_train.py.
What the yardstick is made of: two fp32 evaluations of a bf16-operand net differ by more than fp32 rounding - a value that
lies within fp32 rounding of a bf16 rounding boundary rounds the other way (a step of 2^-8 relative in that operand).  Both the
device and the fp32 restatement have such steps against float64, at elements that depend on the order of their sums, so r32
depends on the host's convolution library (as tests/test_vgg16_train.py's e32 does) and the 32 frames of the batch are there to
give both sides several of them.  A ReLU mask that comes out differently would be a far larger step (measured: 3e-2 on a
gradient), so the net's shifts keep every pre-activation away from zero (``keep_clear_of_zero``) and ``yardstick`` asserts it
with that file's MARGIN_FACTOR = 16.  Measured on the device (ratios device / r32, bound 8): initial weights 1.00 to 1.36,
after the update 0.86 to 2.77; the table is in profiles/conv_bf16_train.md.

Captured against eager, bit for bit: the small net under ``torch.cuda.graph`` (it has no float atomics), before and after a weight
update.  The graph key, ``enable_train_graphs()``, ``apply_update`` and ``check_replays``' allowance run on the FPN detector of
tests/test_train_graphs.py, where only the loss and 16 gradients can be bit-equal.
"""
import numpy as np
import pytest

import bf16_train_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND_FACTOR = 8.0
MARGIN_FACTOR = 16.0
DETECTOR_ALLOWANCE = 4 * 5.8e-3     # the detector's gradients behind float atomics: four times the largest eager-to-eager difference measured
BATCH, MAP_H, MAP_W = 32, 12, 16
_CACHE = {}


@pytest.fixture
def cfg_train():
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.nets import hip_modules
    C.reset_cfg()
    hip_modules.set_net_mode('TRAIN')
    try:
        yield C
    finally:
        C.reset_cfg()
        hip_modules.set_net_mode(None)


def build_modules(seed=11):
    """(conv0, conv0b, block a, block b) on the host, BatchNorms in eval mode with seeded statistics, convolutions trainable."""
    import torch
    import torch.nn as nn
    from faster_rcnn_pytorch_multimodal_amd.nets.resnet import Bottleneck
    torch.manual_seed(seed)
    conv0 = nn.Conv2d(8, 64, 3, padding=1)
    conv0b = nn.Conv2d(64, 64, 1)
    down = nn.Sequential(nn.Conv2d(64, 128, 1, stride=2, bias=False), nn.BatchNorm2d(128))
    a = Bottleneck(64, 32, stride=2, downsample=down)
    b = Bottleneck(128, 32)
    gen = torch.Generator().manual_seed(seed + 1)
    for m in (a, b):
        for bn in [mod for mod in m.modules() if isinstance(mod, nn.BatchNorm2d)]:
            bn.weight.data = 0.5 + torch.rand(bn.weight.shape, generator=gen)
            bn.bias.data = 0.2 * torch.randn(bn.bias.shape, generator=gen)
            bn.running_mean.data = 0.1 * torch.randn(bn.bias.shape, generator=gen)
            bn.running_var.data = 0.5 + torch.rand(bn.bias.shape, generator=gen)
            bn.eval()
            for prm in bn.parameters():
                prm.requires_grad_(False)
    mods = (conv0, conv0b, a, b)
    keep_clear_of_zero(mods)
    return mods


# Every pre-activation of the net is kept well away from zero: channel k of each of the eight layers gets the shift that puts
# its pre-activations at (-1)^k * CLEAR standard deviations from zero (its own statistics over the batch, float64).  Half the
# channels of every map are therefore live at every pixel and half are dead at every pixel: the ReLU masks of both kinds are
# exercised, and no mask can come out differently in two evaluations that differ by rounding - which would change a
# gradient by a whole term, not by rounding (tests/test_vgg16_train.py keeps clear of the same corner by choosing seeds).
# The price: a channel's mask is the same at every pixel, so a mask applied at the wrong PIXEL could not show in this file;
# element-wise masks are tests/test_conv_dgrad_bf16.py's (``act_y`` drawn per element, bit for bit).
CLEAR = 12.0
PRE_LAYERS = ("conv0.bias", "conv0b.bias", "a.bn1.shift", "a.bn2.shift", "a.bn3.shift", "b.bn1.shift", "b.bn2.shift", "b.bn3.shift")


def keep_clear_of_zero(mods):
    import torch
    conv0, conv0b, a, b = mods
    x, _ = case_tensors()
    holders = {"conv0.bias": conv0.bias, "conv0b.bias": conv0b.bias}
    for prefix, blk in (("a", a), ("b", b)):
        for i in (1, 2, 3):
            holders["%s.bn%d.shift" % (prefix, i)] = getattr(blk, "bn%d" % i).bias
    with torch.no_grad():
        for index, name in enumerate(PRE_LAYERS):
            p, _ = restatement_params(mods, torch.float64)
            pre = []
            R.small_net(x.double(), p, True, pre=pre)
            t = pre[index].detach()
            mean, std = t.mean((0, 2, 3)), t.std((0, 2, 3))
            sign = torch.tensor([1.0 if k % 2 == 0 else -1.0 for k in range(t.shape[1])], dtype=torch.float64)
            holders[name].add_((sign * CLEAR * std - mean).to(holders[name]))


def restatement_params(mods, dtype):
    """name -> tensor for R.small_net; the folded scale / shift are formed in fp32 exactly as hip_modules.prepared_conv forms them
    (they are inputs of the function, not part of what is compared)."""
    import torch
    conv0, conv0b, a, b = mods
    p, trained = {}, []
    for name, conv in (("conv0", conv0), ("conv0b", conv0b)):
        for leaf in ("weight", "bias"):
            p["%s.%s" % (name, leaf)] = getattr(conv, leaf).detach().cpu().to(dtype).requires_grad_(True)
            trained.append("%s.%s" % (name, leaf))
    for prefix, blk in (("a", a), ("b", b)):
        pairs = [("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3")]
        layers = [(cn, getattr(blk, cn), bn, getattr(blk, bn)) for cn, bn in pairs]
        if blk.downsample is not None:
            layers.append(("downsample.0", blk.downsample[0], "downsample.1", blk.downsample[1]))
        for cn, conv, bnn, bn in layers:
            p["%s.%s.weight" % (prefix, cn)] = conv.weight.detach().cpu().to(dtype).requires_grad_(True)
            trained.append("%s.%s.weight" % (prefix, cn))
            scale = (bn.weight.detach() / torch.sqrt(bn.running_var.detach() + bn.eps)).float().cpu()
            shift = (bn.bias.detach() - bn.running_mean.detach() * scale.to(bn.bias.device)).float().cpu()
            p["%s.%s.scale" % (prefix, bnn)] = scale.to(dtype)
            p["%s.%s.shift" % (prefix, bnn)] = shift.to(dtype)
    return p, trained


def case_tensors():
    import torch
    gen = torch.Generator().manual_seed(4)
    x = torch.randn((BATCH, 8, MAP_H, MAP_W), generator=gen, dtype=torch.float32)
    g = torch.randn((BATCH, 128, MAP_H // 2, MAP_W // 2), generator=gen, dtype=torch.float32)
    return x, g


def run_restatement(mods, dtype, bf16=True):
    """(output NCHW, {name: gradient}, front-convolution output) of the restatement in ``dtype`` on the host."""
    import torch
    x, g = case_tensors()
    p, trained = restatement_params(mods, dtype)
    stages = []
    out = R.small_net(x.to(dtype), p, bf16, stages=stages)
    grads = torch.autograd.grad((out * g.to(dtype)).sum(), [p[n] for n in trained])
    return out.detach(), dict(zip(trained, [t.detach() for t in grads])), stages[0].detach()


def module_of(mods, name):
    conv0, conv0b, a, b = mods
    if name.startswith("conv0b"):
        return conv0b
    if name.startswith("conv0"):
        return conv0
    mod = a if name.startswith("a.") else b
    for part in name.split(".")[1:-1]:
        mod = mod[int(part)] if part.isdigit() else getattr(mod, part)
    return mod


def run_device(mods, zero=True):
    """(output NCHW, {name: gradient}, front-convolution output) of the package's autograd nodes on the device."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd.nets import autograd_ops as A
    conv0, conv0b, a, b = mods
    x, g = case_tensors()
    xd = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    gd = g.to(DEV).permute(0, 2, 3, 1).contiguous()
    if zero:
        for m in mods:
            m.zero_grad(set_to_none=True)
    front = A.conv_bn_act_train(xd, conv0, None, relu=True)
    t = A.conv_bn_act_train(front, conv0b, None, relu=True)
    out = b(a(t))
    (out * gd).sum().backward()
    A.join_weight_grads(DEV)
    torch.cuda.synchronize()
    _, trained = restatement_params(mods, torch.float32)
    grads = {}
    for name in trained:
        grads[name] = getattr(module_of(mods, name), name.split(".")[-1]).grad.detach().cpu().clone()
    return out.detach().permute(0, 3, 1, 2).cpu(), grads, front.detach().permute(0, 3, 1, 2).cpu()


def device_modules(seed=11):
    mods = build_modules(seed)
    for m in mods:
        m.to(DEV)
    return mods


def rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


def test_switch_absent_and_false_are_the_fp32_step(hip, cfg_train):
    import torch
    mods = device_modules()
    assert cfg_train.cfg.TRAIN.CONV_BF16 is False
    out_f, grads_f, _ = run_device(mods)
    del cfg_train.cfg.TRAIN['CONV_BF16']
    assert 'CONV_BF16' not in cfg_train.cfg.TRAIN
    out_a, grads_a, _ = run_device(mods)
    assert torch.equal(out_f, out_a)
    for name in grads_f:
        assert torch.equal(grads_f[name], grads_a[name]), name
    # and it is the fp32 computation: the plain restatement, to fp32 accuracy
    out64, grads64, _ = run_restatement(mods, torch.float64, bf16=False)
    assert rel(out_f, out64) < 1e-5
    assert all(rel(grads_f[n], grads64[n]) < 1e-5 for n in grads_f)


def test_switch_on_moves_the_eligible_layers_only(hip, cfg_train, monkeypatch):
    """Eligible layers' results differ from fp32; conv0 (C = 8) fed the same input gives the same bits; the launch hooks see
    eight bf16 forwards and filter gradients, seven bf16 data gradients, and in fp32 conv0's forward and filter gradient and
    the one strided 1x1 data gradient (the projection's)."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    mods = device_modules()
    out_f, grads_f, front_f = run_device(mods)
    calls = {}

    def counted(name):
        real = getattr(ops, name)

        def wrapper(*args, **kwargs):
            calls[name] = calls.get(name, 0) + 1
            return real(*args, **kwargs)
        monkeypatch.setattr(ops, name, wrapper)

    for name in ("conv2d_nhwc", "conv2d_nhwc_bf16", "conv2d_bwd_data", "conv2d_bwd_data_bf16", "conv2d_bwd_weight",
                 "conv2d_bwd_weight_bf16", "conv2d_bwd_weight_acc", "conv2d_bwd_weight_acc_bf16", "conv2d_bwd_weight_acc_grouped"):
        counted(name)
    cfg_train.cfg.TRAIN.CONV_BF16 = True
    out_b, grads_b, front_b = run_device(mods)
    assert calls == {"conv2d_nhwc": 1, "conv2d_nhwc_bf16": 8, "conv2d_bwd_data": 1, "conv2d_bwd_data_bf16": 7,
                     "conv2d_bwd_weight": 1, "conv2d_bwd_weight_bf16": 8}, calls
    assert torch.equal(front_f, front_b)
    assert not torch.equal(out_f, out_b)
    for name in grads_f:
        assert not torch.equal(grads_f[name], grads_b[name]), name
    # conv0 outside a TRAIN-mode forward: the switch alone does nothing
    from faster_rcnn_pytorch_multimodal_amd.nets import hip_modules
    hip_modules.set_net_mode('TEST')
    out_t, grads_t, _ = run_device(mods)
    assert torch.equal(out_t, out_f) and all(torch.equal(grads_t[n], grads_f[n]) for n in grads_f)


def yardstick(mods, key):
    import torch
    if key not in _CACHE:
        out64, grads64, _ = run_restatement(mods, torch.float64)
        out32, grads32, _ = run_restatement(mods, torch.float32)
        # the case keeps clear of the ReLU corner: the smallest |pre-activation| against the largest gap between the fp32
        # and the float64 evaluation of a pre-activation, tests/test_vgg16_train.py's MARGIN_FACTOR
        x, _ = case_tensors()
        pre64, pre32 = [], []
        R.small_net(x.double(), restatement_params(mods, torch.float64)[0], True, pre=pre64)
        R.small_net(x.float(), restatement_params(mods, torch.float32)[0], True, pre=pre32)
        smallest = min(float(t.abs().min()) for t in pre64)
        e32 = max(float((u.double() - t).abs().max()) for t, u in zip(pre64, pre32))
        print("%s: smallest |pre-activation| %.3e, largest fp32 - float64 gap of one %.3e" % (key, smallest, e32))
        assert smallest >= MARGIN_FACTOR * e32, (smallest, e32)
        r32 = {"output": rel(out32, out64)}
        r32.update({n: rel(grads32[n], grads64[n]) for n in grads64})
        _CACHE[key] = (out64, grads64, r32)
    return _CACHE[key]


def check_against_restatement(mods, key, got_out, got_grads):
    out64, grads64, r32 = yardstick(mods, key)
    got = {"output": rel(got_out, out64)}
    got.update({n: rel(got_grads[n], grads64[n]) for n in grads64})
    for name in got:
        print("%s %-24s device %.3e  fp32 restatement %.3e  ratio %.2f" % (key, name, got[name], r32[name], got[name] / r32[name]))
    for name in got:
        assert got[name] <= BOUND_FACTOR * r32[name], (name, got[name], r32[name])
    return got


def test_switch_on_is_the_restatement(hip, cfg_train):
    import torch
    mods = device_modules()
    cfg_train.cfg.TRAIN.CONV_BF16 = True
    out_b, grads_b, _ = run_device(mods)
    check_against_restatement(mods, "initial", out_b, grads_b)
    plain64, _, _ = run_restatement(mods, torch.float64, bf16=False)
    assert rel(out_b, plain64) > 1e-4           # two bf16 roundings per product, not fp32 accuracy


def test_bf16_packs_follow_a_weight_update(hip, cfg_train):
    """One gradient step on the accumulated gradients (in place, as the solver's), then the next pass: the restatement on the
    UPDATED weights.  A stale bf16 pack of the filter or of its flipped / transposed form would still compute with the old ones."""
    import torch
    mods = device_modules()
    cfg_train.cfg.TRAIN.CONV_BF16 = True
    run_device(mods)
    before = [p.detach().clone() for m in mods for p in m.parameters() if p.requires_grad]
    with torch.no_grad():                       # a gradient step of a twentieth of each parameter's norm, in place
        for m in mods:
            for p in m.parameters():
                if p.requires_grad:
                    p.add_(p.grad, alpha=-0.05 * float(p.norm() / p.grad.norm()))
    keep_clear_of_zero(mods)                    # (the shifts again, for the new weights: in place too)
    after = [p.detach() for m in mods for p in m.parameters() if p.requires_grad]
    assert all(not torch.equal(b0, a0) for b0, a0 in zip(before, after))
    out_b, grads_b, _ = run_device(mods)
    check_against_restatement(mods, "updated", out_b, grads_b)
    # the same through refresh_derived_weights, the path of a captured step (no Python sees the new versions there)
    from faster_rcnn_pytorch_multimodal_amd.nets.hip_modules import refresh_derived_weights
    with torch.no_grad():
        for m in mods:
            for p in m.parameters():
                if p.requires_grad:
                    p.mul_(1.25)
    for m in mods:
        assert refresh_derived_weights(m) > 0
    packs = [(m2.__dict__["_frcnn_bf16"][1][0], m2.__dict__["_frcnn_prepared"][1][0]) for m in mods[2:] for m2 in m.modules()
             if "_frcnn_bf16" in m2.__dict__]
    assert len(packs) == 7
    for packed, w_krsc in packs:
        assert torch.equal(packed.view(torch.bfloat16).float(), w_krsc.to(torch.bfloat16).float())
    tpacks = [(m2.__dict__["_frcnn_dgrad_bf16"][1][0], m2.__dict__["_frcnn_wt"][1][0]) for m in mods[2:] for m2 in m.modules()
              if "_frcnn_dgrad_bf16" in m2.__dict__]
    assert len(tpacks) == 6                      # the projection's strided 1x1 data gradient has no bf16 pack
    for packed, w_t in tpacks:
        assert torch.equal(packed.view(torch.bfloat16).float(), w_t.to(torch.bfloat16).float())


def test_captured_small_net_is_the_eager_pass_bit_for_bit(hip, cfg_train):
    """The small net has no float atomic anywhere: every kernel on its path is deterministic, so a captured pass must give the
    eager pass's output and EVERY parameter gradient bit for bit.  Forward and backward are captured under ``torch.cuda.graph``
    with the schedule a captured step uses (filter gradients added into ``param.grad`` in line) after one eager pass under the
    same schedule; the replay is compared with that eager pass and with the plain eager pass (gradients through autograd) -
    before and after an in-place weight update followed by ``refresh_derived_weights``, which is all a replayed graph gets:
    it reads the filters, their flipped / transposed forms and the bf16 packs of both by address."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import capture
    from faster_rcnn_pytorch_multimodal_amd.nets import autograd_ops as A
    from faster_rcnn_pytorch_multimodal_amd.nets.hip_modules import refresh_derived_weights
    mods = device_modules()
    conv0, conv0b, a, b = mods
    cfg_train.cfg.TRAIN.CONV_BF16 = True
    x, g = case_tensors()
    xd = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    gd = g.to(DEV).permute(0, 2, 3, 1).contiguous()
    params = [p for m in mods for p in m.parameters() if p.requires_grad]
    _, trained = restatement_params(mods, torch.float32)
    schedule = A.WgradSchedule(accumulate=True, side_stream=False, grouped=False, bn_stat_sink=None)

    def one_pass():
        front = A.conv_bn_act_train(xd, conv0, None, relu=True)
        out = b(a(A.conv_bn_act_train(front, conv0b, None, relu=True)))
        (out * gd).sum().backward()
        A.join_weight_grads(DEV)
        return out.detach()

    def gradients():
        torch.cuda.synchronize()
        return {n: getattr(module_of(mods, n), n.split(".")[-1]).grad.detach().clone() for n in trained}

    def same(got, want, what):
        assert torch.equal(got[0], want[0]), what
        for n in trained:
            assert torch.equal(got[1][n], want[1][n]), (what, n)

    plain = [None, None]
    out_p, grads_p, _ = run_device(mods)                      # the plain eager pass: gradients returned to autograd
    plain[0] = (out_p, grads_p)
    for p in params:                                          # a captured step's gradient buffers: in place from here on
        p.grad = torch.zeros_like(p)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), A.wgrad_schedule(schedule):
        eager = (one_pass().clone(), gradients())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same((eager[0].permute(0, 3, 1, 2).cpu(), {n: t.cpu() for n, t in eager[1].items()}), plain[0], "in-place eager against plain eager")
    torch._foreach_zero_([p.grad for p in params])
    graph = torch.cuda.CUDAGraph()
    with A.wgrad_schedule(schedule), capture(graph):
        out_static = one_pass()
    for step in range(2):
        torch._foreach_zero_([p.grad for p in params])
        out_static.fill_(float("nan"))
        graph.replay()
        same((out_static, gradients()), eager, "replay %d against the eager pass" % step)
    before = eager
    # the update, in place, and what a captured step gets afterwards
    with torch.no_grad():
        for p in params:
            p.add_(p.grad, alpha=-0.05 * float(p.norm() / p.grad.norm()))
    for m in mods:
        assert refresh_derived_weights(m) > 0
    torch._foreach_zero_([p.grad for p in params])
    with A.wgrad_schedule(schedule):
        eager = (one_pass().clone(), gradients())
    assert not torch.equal(eager[0], before[0]) and all(not torch.equal(eager[1][n], before[1][n]) for n in trained)
    torch._foreach_zero_([p.grad for p in params])
    out_static.fill_(float("nan"))
    graph.replay()
    same((out_static, gradients()), eager, "replay after the update against the eager pass")


# ---- the detector: captured step, graph key, update -------------------------------------------------------------------------
def test_graph_key_carries_the_switch(hip):
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import train_graph
    C.reset_cfg()
    try:
        off = train_graph.capture_switches()
        C.cfg.TRAIN.CONV_BF16 = True
        on = train_graph.capture_switches()
        del C.cfg.TRAIN['CONV_BF16']
        absent = train_graph.capture_switches()
        assert off != on and absent == off
    finally:
        C.reset_cfg()


def test_captured_step_equals_the_eager_step_and_follows_the_update(hip):
    """FPN detector (tests/test_train_graphs.py's), switch on, three steps with a weight update after each.

    What can be bit-equal is: the loss, and the 16 gradients of the heads behind the RoIAlign and of the RPN's own layers, which
    two EAGER steps on the same frame and seeds give bit for bit.  The others lie behind the float atomics of the RoIAlign backward and of the RPN's patch scatter, whose summation order varies
    from run to run (include/frcnn_hip.h says so): two eager fp32 steps of this detector already differ in 105 of its 121
    gradients, by up to 5e-7 of a tensor's largest element, and with bf16 operands that last-bit difference moves roundings
    further down the backward pass - two eager steps then differ by 1e-7 to 5.8e-3, run by run (twelve pairs,
    profiles/conv_bf16_train.md): either a rounding moves and the difference spreads, or none does, so one pair of eager runs is
    no yardstick for another.  This comparison is a supplement to ``test_captured_small_net_is_the_eager_pass_bit_for_bit``,
    which has no atomics and asks for every bit; here those 105 gradients get a MEASURED allowance, DETECTOR_ALLOWANCE = four
    times the largest difference seen between two eager steps.
    Before each update the eager gradients are copied into the captured net's buffers, so both nets keep identical weights:
    the next captured step's loss is again the eager step's bit for bit only if apply_update re-packed the bf16 filters in
    place (the replayed graph reads them by address).  The step stays ONE chain (train_graph.check_replays knows the switch),
    and toggling the switch captures another graph."""
    import torch
    import test_gpu_parity as T
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd import ops
    try:
        net_e, _ = T._build_fpn_pair(seed=23)
        net_g, _ = T._build_fpn_pair(seed=23)
        C.cfg.TRAIN.CONV_BF16 = True
        data, info, gt, _, _ = T._fpn_case()
        for n in (net_e, net_g):
            n.train()
        net_g.enable_train_graphs(True)
        opts = [torch.optim.SGD([p for p in n.parameters() if p.requires_grad], lr=1e-3) for n in (net_e, net_g)]
        seen = {}
        real = ops.conv2d_bwd_weight_acc_bf16

        def counted(*args, **kwargs):
            seen["acc_bf16"] = seen.get("acc_bf16", 0) + 1
            return real(*args, **kwargs)
        ops.conv2d_bwd_weight_acc_bf16 = counted

        bound = DETECTOR_ALLOWANCE

        def grads_of(net):
            return {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.requires_grad and p.grad is not None}

        def deviation(a, b):
            return float((a - b).abs().max() / a.abs().max().clamp_min(1e-30))

        try:
            for o in opts:
                o.zero_grad(set_to_none=False)
            for it in range(3):
                blobs = {"data": data * (1.0 + 0.1 * it), "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
                torch.manual_seed(300 + it)                 # graph net first: its warm-up tunes the plans both then use
                loss_g = net_g.train_step(blobs, opts[1], update_weights=False)
                eager = []
                for rep in range(2):
                    opts[0].zero_grad(set_to_none=False)
                    torch.manual_seed(300 + it)
                    loss_e = net_e.train_step(blobs, opts[0], update_weights=False)
                    torch.cuda.synchronize()
                    eager.append(grads_of(net_e))
                    assert loss_e == loss_g, (it, rep, loss_e, loss_g)
                captured = grads_of(net_g)
                assert set(eager[1]) <= set(captured)      # (the captured net holds zero buffers for parameters no loss reaches)
                # the heads behind the RoIAlign and the RPN's own layers: no float atomic on the way to their gradients
                fixed = [n for n in eager[0] if n.startswith(("cls_score_net", "bbox_pred_net", "t_fc", "rpn_"))]
                loose = [n for n in eager[0] if n not in fixed]
                assert len(fixed) == 16 and len(loose) > 90, (fixed, len(loose))
                for n in fixed:
                    assert torch.equal(eager[0][n], eager[1][n]), (it, n)
                    assert torch.equal(captured[n], eager[1][n]), (it, n)
                worst_ee = max([deviation(eager[1][n], eager[0][n]) for n in loose] + [0.0])
                worst_ge = max([deviation(eager[1][n], captured[n]) for n in loose] + [0.0])
                print("step %d: %d gradients bit-equal, %d behind float atomics: captured-eager %.3e, eager-eager %.3e"
                      % (it, len(fixed), len(loose), worst_ge, worst_ee))
                assert worst_ge <= bound, (it, worst_ge, bound)
                # identical gradients into both updates: the nets keep identical weights
                with torch.no_grad():
                    for (_, pe), (_, pg) in zip(net_e.named_parameters(), net_g.named_parameters()):
                        if pe.requires_grad and pe.grad is not None:
                            pg.grad.copy_(pe.grad)
                net_e.apply_update(opts[0], in_place=False)
                net_g.apply_update(opts[1], in_place=True)
                opts[0].zero_grad(set_to_none=False)
        finally:
            ops.conv2d_bwd_weight_acc_bf16 = real
        assert seen.get("acc_bf16", 0) > 0              # the captured step's filter gradients did run the bf16 kernel
        assert len(net_g._train_graphs) == 1
        assert all(r.inline for r in net_g._train_graphs.values())
        C.cfg.TRAIN.CONV_BF16 = False
        blobs = {"data": data, "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
        net_g.train_step(blobs, opts[1], update_weights=False)
        assert len(net_g._train_graphs) == 2
    finally:
        C.reset_cfg()


def test_check_replays_allowance_is_a_constant_and_still_refuses(hip):
    """``train_graph.check_replays`` on replays that differ by a chosen amount: without the switch it refuses above 1e-3 as it
    always did; under the switch it refuses above REPLAY_TOLERANCE_CONV_BF16, a constant within five times the measured 5.8e-3."""
    import types
    import torch
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import train_graph
    assert train_graph.REPLAY_TOLERANCE == 1e-3
    assert 5.8e-3 < train_graph.REPLAY_TOLERANCE_CONV_BF16 <= 5 * 5.8e-3
    net = types.SimpleNamespace(_device=DEV)
    base = torch.linspace(-1.0, 1.0, 64, device=DEV)            # largest element 1: a deviation is its own relative size
    grads = [torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)]

    def runner_with(deviation):
        calls = [0]

        def run(blobs):
            calls[0] += 1
            grads[0].add_(base)
            grads[1].add_(base)
            if calls[0] == 3:                                   # the third replay is off in one element of the second tensor
                grads[1][5] += deviation
            return None
        return types.SimpleNamespace(run=run, bn_modules=[], node_kinds={})

    C.reset_cfg()
    try:
        for switch, tol in ((False, train_graph.REPLAY_TOLERANCE), (True, train_graph.REPLAY_TOLERANCE_CONV_BF16)):
            C.cfg.TRAIN.CONV_BF16 = switch
            train_graph.check_replays(net, runner_with(0.8 * tol), None, grads)
            with pytest.raises(train_graph.ReplayMismatch):
                train_graph.check_replays(net, runner_with(1.25 * tol), None, grads)
            assert all(float(t.abs().max()) == 0.0 for t in grads)         # the check leaves no trace
    finally:
        C.reset_cfg()
