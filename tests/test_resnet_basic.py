"""nets.imagenet.imagenet(num_layers=18 / 34): the BasicBlock ResNet detectors (the reference's ``--net res34``), inference.

Reference: tests/resnet_basic_restatement.py - the nets restated with torch functional calls from the reference's BasicBlock
and the published torchvision layout, run in fp32 and float64 on the CPU with seeded weights.  The block's own arithmetic is
pinned to the reference's ``BasicBlock`` class by tests/golden/basicblock.npz (tests/golden/make_golden_basicblock.py); the
detector as a whole is PARITY UNPINNED: ``resnet18()`` / ``resnet34()`` raise TypeError in the reference, its ``ResNetWrapper``
cannot put a BasicBlock layer4 at stride 1, and its imagenet.py hard-codes the Bottleneck widths.

Bounds.  e32 = max |restatement fp32 - restatement float64| on the tensor of the check is the error an fp32 evaluation of this
function has on this input.  The device sums the same fp32 products in MFMA / Winograd / split-K order: 8 * e32, the factor and
form tests/test_vgg16.py and tests/test_mobilenet.py use.  A wrong stride, a missing shortcut or a residual added behind the
ReLU is an error of order 0.1 - 1.  The GPU comparisons run under the default algorithm (no plan: the closing convolution of a
block is the implicit GEMM with the residual) and under forced Winograd (it is the residual Winograd output transform).
"""
import numpy as np
import pytest

import resnet_basic_restatement as R

DEV = "cuda:0"
DEPTHS = (18, 34)
ALGOS = (0, 2)
_CACHE = {}

# torchvision's resnet18 without fc, written out: (key, shape) in module order
_BN = lambda p, c: [(p + ".weight", (c,)), (p + ".bias", (c,)), (p + ".running_mean", (c,)), (p + ".running_var", (c,)),
                    (p + ".num_batches_tracked", ())]
RESNET18 = (
    [("conv1.weight", (64, 3, 7, 7))] + _BN("bn1", 64)
    + [("layer1.0.conv1.weight", (64, 64, 3, 3))] + _BN("layer1.0.bn1", 64)
    + [("layer1.0.conv2.weight", (64, 64, 3, 3))] + _BN("layer1.0.bn2", 64)
    + [("layer1.1.conv1.weight", (64, 64, 3, 3))] + _BN("layer1.1.bn1", 64)
    + [("layer1.1.conv2.weight", (64, 64, 3, 3))] + _BN("layer1.1.bn2", 64)
    + [("layer2.0.conv1.weight", (128, 64, 3, 3))] + _BN("layer2.0.bn1", 128)
    + [("layer2.0.conv2.weight", (128, 128, 3, 3))] + _BN("layer2.0.bn2", 128)
    + [("layer2.0.downsample.0.weight", (128, 64, 1, 1))] + _BN("layer2.0.downsample.1", 128)
    + [("layer2.1.conv1.weight", (128, 128, 3, 3))] + _BN("layer2.1.bn1", 128)
    + [("layer2.1.conv2.weight", (128, 128, 3, 3))] + _BN("layer2.1.bn2", 128)
    + [("layer3.0.conv1.weight", (256, 128, 3, 3))] + _BN("layer3.0.bn1", 256)
    + [("layer3.0.conv2.weight", (256, 256, 3, 3))] + _BN("layer3.0.bn2", 256)
    + [("layer3.0.downsample.0.weight", (256, 128, 1, 1))] + _BN("layer3.0.downsample.1", 256)
    + [("layer3.1.conv1.weight", (256, 256, 3, 3))] + _BN("layer3.1.bn1", 256)
    + [("layer3.1.conv2.weight", (256, 256, 3, 3))] + _BN("layer3.1.bn2", 256)
    + [("layer4.0.conv1.weight", (512, 256, 3, 3))] + _BN("layer4.0.bn1", 512)
    + [("layer4.0.conv2.weight", (512, 512, 3, 3))] + _BN("layer4.0.bn2", 512)
    + [("layer4.0.downsample.0.weight", (512, 256, 1, 1))] + _BN("layer4.0.downsample.1", 512)
    + [("layer4.1.conv1.weight", (512, 512, 3, 3))] + _BN("layer4.1.bn1", 512)
    + [("layer4.1.conv2.weight", (512, 512, 3, 3))] + _BN("layer4.1.bn2", 512))


def state(depth, seed=R.SEED):
    """The seeded weights - made once per (depth, seed), never modified."""
    if (depth, seed) not in _CACHE:
        _CACHE[(depth, seed)] = R.seeded_state(depth, seed)
    return _CACHE[(depth, seed)]


def head_input():
    return np.random.default_rng(1).standard_normal((1, 3, 64, 96)).astype(np.float32)


def pooled_input():
    return np.random.default_rng(2).random((3, 256, 7, 7)).astype(np.float32)


def restated(fn, depth, x, seed=R.SEED):
    """([float64 stages], [e32 per stage]) of ``fn`` = R.head / R.tail on the NCHW numpy array ``x``."""
    import torch
    s64, s32 = [], []
    with torch.no_grad():
        fn(state(depth, seed), depth, torch.from_numpy(np.asarray(x, np.float64)), s64)
        fn(state(depth, seed), depth, torch.from_numpy(np.asarray(x, np.float32)), s32)
    s64 = [t.numpy() for t in s64]
    return s64, [float(np.abs(b.numpy().astype(np.float64) - a).max()) for a, b in zip(s64, s32)]


def cached_restated(name, fn, depth, make):
    if (name, depth) not in _CACHE:
        _CACHE[(name, depth)] = restated(fn, depth, make())
    return _CACHE[(name, depth)]


def build_net(depth, device=None, seed=3):
    import torch
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
    torch.manual_seed(seed)
    net = imagenet(num_layers=depth)
    net.create_architecture(2, tag='default', anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
    net.resnet.load_state_dict(state(depth), strict=True)
    net.eval()
    if device is not None:
        net._device = device
        net.to(device)
    return net


@pytest.fixture
def cfg_reset():
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    C.reset_cfg()
    C.cfg.NET_TYPE = "image"
    try:
        yield C
    finally:
        C.reset_cfg()


# ---- CPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
def test_constructs_with_torchvisions_keys_and_the_blocks_widths(cfg_reset, depth):
    import torch.nn as nn
    from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
    from faster_rcnn_pytorch_multimodal_amd.nets.resnet import BasicBlock
    net = build_net(depth)
    sd = net.state_dict()
    body = [(k[len("resnet."):], tuple(v.shape)) for k, v in sd.items() if k.startswith("resnet.")]
    assert body == R.key_shapes(depth)
    if depth == 18:
        assert body == RESNET18
    assert [len(getattr(net.resnet, "layer%d" % i)) for i in (1, 2, 3, 4)] == list(R.LAYERS[depth])
    assert BasicBlock.expansion == 1
    for i in (1, 2, 3, 4):
        for j, blk in enumerate(getattr(net.resnet, "layer%d" % i)):
            assert type(blk) is BasicBlock
            names = [n for n, _ in blk.named_children()]
            assert names == ["conv1", "bn1", "conv2", "bn2"] + (["downsample"] if j == 0 and i > 1 else []), (i, j, names)
            assert tuple(blk.conv2.stride) == (1, 1) and tuple(blk.conv2.padding) == (1, 1) and blk.conv2.bias is None
            assert isinstance(blk.bn2, nn.BatchNorm2d)
    # the heads and the RPN: the keys of the other depths, the widths of the block's expansion
    res = imagenet(num_layers=50)
    res.create_architecture(2, tag='default')
    assert [k for k in sd if not k.startswith("resnet.")] == [k for k in res.state_dict() if not k.startswith("resnet.")]
    assert (net._feat_stride, net._net_conv_channels, net._roi_pooling_channels, net._fc7_channels,
            net._det_net_channels) == (16, 256, 256, 512, 512)
    assert tuple(sd["rpn_net.weight"].shape) == (512, 256, 3, 3) and tuple(sd["cls_score_net.weight"].shape) == (2, 512)
    assert tuple(sd["bbox_pred_net.weight"].shape) == (8, 512)


@pytest.mark.parametrize("depth", DEPTHS)
def test_strides_layer4_runs_at_stride_1_without_fpn(cfg_reset, depth):
    net = build_net(depth)
    r = net.resnet
    assert tuple(r.layer1[0].conv1.stride) == (1, 1) and r.layer1[0].downsample is None
    for name in ("layer2", "layer3"):
        first = getattr(r, name)[0]
        assert tuple(first.conv1.stride) == (2, 2) and tuple(first.downsample[0].stride) == (2, 2) and first.stride == 2
        assert all(tuple(b.conv1.stride) == (1, 1) and b.downsample is None for b in list(getattr(r, name))[1:])
    first = r.layer4[0]
    assert tuple(first.conv1.stride) == (1, 1) and tuple(first.downsample[0].stride) == (1, 1) and first.stride == 1
    assert tuple(first.downsample[0].kernel_size) == (1, 1)
    assert all(tuple(b.conv2.stride) == (1, 1) for layer in (r.layer1, r.layer2, r.layer3, r.layer4) for b in layer)


def test_restated_block_equals_the_references_basicblock(golden_dir):
    """tests/golden/basicblock.npz holds the outputs of the reference's own BasicBlock class (stride 1 without a shortcut,
    stride 2 with one) on a seeded (2,8,6,5) input: the float64 restatement is within 8 e32 of them (e32: the fp32
    restatement's own distance from float64 on that output), and the weights are re-made from the stored seeds."""
    import os
    import torch
    g = np.load(os.path.join(golden_dir, "basicblock.npz"))
    assert g["x"].shape == (2, 8, 6, 5)
    for name, inplanes, planes, stride, shape in (("plain", 8, 8, 1, (2, 8, 6, 5)), ("down", 8, 16, 2, (2, 16, 3, 3))):
        shapes = R.block_shapes("", inplanes, planes, name == "down")
        assert [k for k, _ in shapes] == list(g["keys_" + name])
        st = R.seeded_from_shapes(shapes, int(g["seed_" + name]))
        with torch.no_grad():
            y64 = R.block(st, "", torch.from_numpy(g["x"]).double(), stride).numpy()
            y32 = R.block(st, "", torch.from_numpy(g["x"]).float(), stride).numpy()
        want = g["y_" + name]
        assert want.shape == shape == y64.shape
        e32 = float(np.abs(y32.astype(np.float64) - y64).max())
        err = float(np.abs(want.astype(np.float64) - y64).max())
        print("basicblock %s: |reference fp32 - restatement float64| %.3g = %.2f e32" % (name, err, err / e32))
        assert 0 < e32 < 1e-5 and err <= 8 * e32 and float((want > 0).mean()) > 0.25


def test_what_is_not_built_raises(cfg_reset):
    from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
    from faster_rcnn_pytorch_multimodal_amd.nets.lidarnet import lidarnet
    cfg = cfg_reset.cfg
    net = build_net(18)
    blob, info = np.zeros((1, 32, 32, 3), np.float32), np.array([0, 32, 0, 32, 0, 0, 1.0], np.float32)
    with pytest.raises(NotImplementedError, match="inference only"):
        net.forward(blob, info, np.zeros((1, 5), np.float32), None, mode='TRAIN')
    with pytest.raises(NotImplementedError, match="training nodes"):
        net(blob, info, np.zeros((1, 5), np.float32))                      # the default mode is TRAIN
    for depth in DEPTHS:
        for set_flag, word in ((lambda: setattr(cfg, 'USE_FPN', True), "USE_FPN"),
                               (lambda: cfg.UC.__setitem__('EN_BBOX_ALEATORIC', True), "EN_BBOX_ALEATORIC"),
                               (lambda: cfg.UC.__setitem__('EN_CLS_EPISTEMIC', True), "EN_CLS_EPISTEMIC"),
                               (lambda: cfg.UC.__setitem__('EN_RPN_CLS_ALEATORIC', True), "EN_RPN_CLS_ALEATORIC")):
            cfg_reset.reset_cfg()
            cfg.NET_TYPE = "image"
            set_flag()
            with pytest.raises(NotImplementedError, match=word):
                imagenet(num_layers=depth)
        cfg_reset.reset_cfg()
        cfg.NET_TYPE = "lidar"
        with pytest.raises(NotImplementedError, match="BasicBlock"):
            lidarnet(num_layers=depth)
    cfg_reset.reset_cfg()
    cfg.NET_TYPE = "image"
    imagenet(num_layers=50)                                                # the other depths are as they were
    with pytest.raises(NotImplementedError, match="resnet depth 20"):
        imagenet(num_layers=20)._build_resnet()


def test_only_basicblock_passes_the_new_keyword():
    """``winograd_residual`` defaults to off in conv_forward / conv_bn_act and exactly one call site turns it on: the existing
    nets (the benchmark's frame among them) keep the route they had."""
    import inspect
    import os
    import re
    from faster_rcnn_pytorch_multimodal_amd.nets import hip_modules
    for fn in (hip_modules.conv_forward, hip_modules.conv_bn_act):
        assert inspect.signature(fn).parameters["winograd_residual"].default is False
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(hip_modules.__file__)))
    users = []
    for folder, _, files in os.walk(pkg):
        for name in files:
            if name.endswith(".py"):
                with open(os.path.join(folder, name)) as f:
                    text = f.read()
                users += [os.path.relpath(os.path.join(folder, name), pkg)] * len(re.findall(r"winograd_residual\s*=\s*True", text))
    assert users == [os.path.join("nets", "resnet.py")], users


def test_load_pretrained_cnn_takes_a_torchvision_keyed_state_dict(cfg_reset):
    import torch
    net = build_net(18)
    other = {k: (v + 1 if v.dtype.is_floating_point else v) for k, v in state(18).items()}
    other["fc.weight"] = torch.zeros(1000, 512)                           # a torchvision checkpoint carries its classifier
    other["fc.bias"] = torch.zeros(1000)
    net.load_pretrained_cnn(other)
    got = net.resnet.state_dict()
    assert all(torch.equal(got[k], other[k]) for k in state(18))


@pytest.mark.parametrize("depth", DEPTHS)
def test_no_stage_of_the_restatement_is_dead(depth):
    """The maps the comparisons below run on: 64x96 -> 16x24 behind the stem -> 16x24, 8x12, 4x6; the tail on 7x7."""
    h64, he = cached_restated("head", R.head, depth, head_input)
    t64, te = cached_restated("tail", R.tail, depth, pooled_input)
    assert [s.shape for s in h64] == [(1, 64, 16, 24), (1, 64, 16, 24), (1, 128, 8, 12), (1, 256, 4, 6)]
    assert [s.shape for s in t64] == [(3, 512, 7, 7), (3, 512)]
    for i, (s, e) in enumerate(zip(h64 + t64, he + te)):
        pos, rms = float((s > 0).mean()), float(np.sqrt((s * s).mean()))
        print("depth %d stage %d %-18s positive %.3f rms %.3f e32 %.3g" % (depth, i, s.shape, pos, rms, e))
        assert pos >= 0.25 and 0.2 < rms < 8.0 and 0 < e < 1e-4, i


# ---- GPU ------------------------------------------------------------------------------------------------------------
INFO = np.array([0, 96, 0, 64, 0, 0, 1.0], np.float32)
KEYS = ('rois', 'rois_count', 'cls_score', 'cls_prob', 'bbox_pred', 'pred_boxes')


def _frame(rng, h=64, w=96):
    return rng.standard_normal((1, h, w, 3)).astype(np.float32)


@pytest.fixture
def algo(hip):
    """set_conv_algo for the body, the default and an empty plan cache afterwards."""
    from faster_rcnn_pytorch_multimodal_amd import ops

    def restore():
        ops.set_conv_algo(0)
        assert hip.frcnn_conv2d_clear_plans() == 0
    restore()
    try:
        yield ops.set_conv_algo
    finally:
        restore()


def _winograd_res_calls(monkeypatch):
    """Counts the calls that reach ops.conv2d_nhwc_winograd_res."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    calls = []
    real = ops.conv2d_nhwc_winograd_res

    def counted(*a, **kw):
        calls.append(tuple(a[0].shape))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "conv2d_nhwc_winograd_res", counted)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ALGOS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_stages_tail_and_fc7_against_float64(hip, cfg_reset, algo, monkeypatch, depth, mode):
    """The stem and layer1 .. layer3 on the (1,3,64,96) input, layer4 and fc7 on a (3,256,7,7) U(0,1) pooled input: every
    stage max |device - float64| <= 8 * e32 of that stage."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.nets.hip_modules import set_net_mode, to_nhwc
    algo(mode)
    calls = _winograd_res_calls(monkeypatch)
    s64, e32 = cached_restated("head", R.head, depth, head_input)
    t64, te32 = cached_restated("tail", R.tail, depth, pooled_input)
    net = build_net(depth, DEV)
    net._mode = 'TEST'
    set_net_mode('TEST')
    with torch.no_grad():
        x = ops.pad_channels(torch.from_numpy(np.ascontiguousarray(head_input().transpose(0, 2, 3, 1))).to(DEV), 4)
        head = net._layers['head']
        got = [head.stem(x)]
        for stage in head.stages:
            got.append(stage(got[-1]))
        net._predictions = {'rois': torch.zeros((3, 5), device=DEV)}
        pooled = torch.from_numpy(pooled_input()).to(DEV)
        layer4 = net._layer4(to_nhwc(pooled))
        fc7 = net._head_to_tail(pooled)
        net._pyramid = None
        assert not net._projected_head_ok()                        # layer4[0].conv1 is 3x3: nothing to move before the pooling
        torch.cuda.synchronize()
    assert tuple(fc7.shape) == (3, 512) and net._predictions['_tail']['fc7'] is fc7
    assert len(calls) == sum(R.LAYERS[depth]) + R.LAYERS[depth][3]     # every block's closing convolution, layer4 twice
    names = ["stem", "layer1", "layer2", "layer3", "layer4", "fc7"]
    got = [t.permute(0, 3, 1, 2) for t in got] + [layer4.permute(0, 3, 1, 2), fc7]
    errs = []
    for name, g, want, e in zip(names, got, s64 + t64, e32 + te32):
        g = g.cpu().numpy().astype(np.float64)
        assert g.shape == want.shape, name
        err = float(np.abs(g - want).max())
        errs.append((name, err, e))
        print("resnet%d %-6s %-18s (algo %d): max |device - float64| %.3g = %.2f e32 (e32 %.3g)"
              % (depth, name, want.shape, mode, err, err / e, e))
    for name, err, e in errs:
        assert err <= 8 * e, (name, err, e)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ALGOS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_whole_frame_stage_by_stage(hip, cfg_reset, algo, depth, mode):
    """forward(mode='TEST') and test_frame on a 64x96 frame (RPN through the heads; the per-class filter through
    detect_frame_device); every stage of the restatement is fed the device's previous stage."""
    import torch
    import torch.nn.functional as F
    from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device
    cfg_reset.cfg.TEST.RPN_POST_NMS_TOP_N = 50
    algo(mode)
    net = build_net(depth, DEV)
    blob = _frame(np.random.default_rng(1))
    with torch.no_grad():
        rois, cls_prob, bbox_pred = net.forward(blob, INFO, None, None, mode='TEST')
        p = dict(net._predictions)
        n = int(p['rois_count'].item())
        assert 0 < n <= 50 and tuple(rois.shape) == (50, 5)
        assert tuple(cls_prob.shape) == (50, 2) and tuple(bbox_pred.shape) == (50, 8) and tuple(p['pred_boxes'].shape) == (50, 8)
        net_conv = net._act_summaries['conv']
        assert tuple(net_conv.shape) == (1, 4, 6, 256)
        s64, e32 = restated(R.head, depth, blob.transpose(0, 3, 1, 2))
        err = float(np.abs(net_conv.permute(0, 3, 1, 2).cpu().numpy().astype(np.float64) - s64[-1]).max())
        print("resnet%d frame net_conv (algo %d): %.3g = %.2f e32" % (depth, mode, err, err / e32[-1]))
        assert float((s64[-1] > 0).mean()) >= 0.25 and err <= 8 * e32[-1]
        # the tail on the device's own pool5
        fc7_frame = p['_tail']['fc7']
        pool5 = net._crop_pool_layer(net_conv.permute(0, 3, 1, 2), rois)
        assert tuple(pool5.shape) == (50, 256, 7, 7)
        fc7 = net._head_to_tail(pool5)
        assert tuple(fc7.shape) == (50, 512) and torch.equal(fc7, fc7_frame)
        t64, e32t = restated(R.tail, depth, pool5[:n].cpu().numpy())
        err = float(np.abs(fc7[:n].cpu().numpy().astype(np.float64) - t64[-1]).max())
        print("resnet%d frame fc7 (algo %d): %.3g = %.2f e32" % (depth, mode, err, err / e32t[-1]))
        assert err <= 8 * e32t[-1]
        # the heads on the device's own fc7
        f = fc7_frame[:n].cpu()
        score = F.linear(f, net.cls_score_net.weight.cpu(), net.cls_score_net.bias.cpu())
        np.testing.assert_allclose(cls_prob[:n].cpu().numpy(), F.softmax(score, 1).numpy(), rtol=0, atol=1e-4)
        np.testing.assert_allclose(bbox_pred[:n].cpu().numpy(),
                                   F.linear(f, net.bbox_pred_net.weight.cpu(), net.bbox_pred_net.bias.cpu()).numpy(), rtol=0, atol=1e-4)
        # test_frame: exactly n rows, like the reference
        cls_score, prob, boxes, rois_n, unc = net.test_frame(blob, INFO)
        assert tuple(cls_score.shape) == (n, 2) and tuple(prob.shape) == (n, 2) and tuple(boxes.shape) == (n, 8)
        assert tuple(rois_n.shape) == (n, 5) and unc == {}
        assert torch.equal(prob, cls_prob[:n]) and torch.equal(rois_n, rois[:n])
        # the per-class filter on the same frame
        dets, counts = detect_frame_device(net, blob, INFO, thresh=0.0, max_dets=100)
        torch.cuda.synchronize()
        k = int(counts[1])
        assert int(counts[0]) == 0 and 0 < k <= n
        kept = dets[1, :k].cpu().numpy()
        assert np.isfinite(kept).all() and (kept[:, 4] >= 0).all() and (kept[:, 4] <= 1).all()
        assert (np.diff(kept[:, 4]) <= 0).all() or k == 1                   # sorted by score
        assert float(kept[:, 4].max()) <= float(prob[:, 1].max()) + 1e-6


def _eager(net, blob, info):
    import torch
    with torch.no_grad():
        net.forward(blob, info, None, None, mode='TEST')
    torch.cuda.synchronize()
    p = net._predictions
    return {k: p[k].clone() for k in KEYS}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ALGOS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_captured_frame_replays_the_eager_bits_and_follows_new_weights(hip, cfg_reset, algo, depth, mode):
    import torch
    cfg_reset.cfg.TEST.RPN_POST_NMS_TOP_N = 50
    algo(mode)
    net = build_net(depth, DEV)
    rng = np.random.default_rng(2)
    frames = [_frame(rng), _frame(rng)]
    net.enable_frame_graphs()
    pool = net.frame_pool(streams=1, autotune=False)
    runner = pool.runner(frames[0].shape, INFO, with_filter=False)
    assert runner is not None and runner.graph is not None and pool.stats['captures'] == 1

    def replay(frame):
        for k in KEYS:                                      # poison: a replay that did not run leaves no plausible result
            runner.predictions[k].fill_(-7 if runner.predictions[k].dtype != torch.float32 else float('nan'))
        runner.run(frame)
        torch.cuda.synchronize()
        return {k: runner.predictions[k].clone() for k in KEYS}

    def check_equal(a, b):
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k

    eager = [_eager(net, f, INFO) for f in frames]
    assert int(eager[0]['rois_count']) > 0 and not torch.equal(eager[0]['cls_prob'], eager[1]['cls_prob'])
    for _ in range(2):
        for f, e in zip(frames, eager):
            check_equal(replay(f), e)
    # the same graph after an IN-PLACE update of a closing convolution's filter and of other seeded weights: the KRSC filters
    # and (forced Winograd) the transformed filters U are re-derived into the storage the graph reads
    conv2 = net.resnet.layer2[1].conv2
    if mode == 2:
        u_ptr = conv2.__dict__['_frcnn_winograd'][1][0].data_ptr()
    with torch.no_grad():
        conv2.weight.mul_(-1.5)
        net.resnet.layer4[0].conv2.weight.add_(0.01)
    pool.sync_weights()
    assert pool.stats['refreshes'] == 1 and pool.stats['invalidations'] == 0 and pool.stats['captures'] == 1
    if mode == 2:
        from faster_rcnn_pytorch_multimodal_amd import ops
        from faster_rcnn_pytorch_multimodal_amd.nets.hip_modules import prepared_conv
        u = conv2.__dict__['_frcnn_winograd'][1][0]
        assert u.data_ptr() == u_ptr and torch.equal(u, ops.winograd_filter(prepared_conv(conv2, net.resnet.layer2[1].bn2)[0]))
    after = replay(frames[0])
    assert not torch.equal(after['cls_score'], eager[0]['cls_score'])
    check_equal(after, _eager(net, frames[0], INFO))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ALGOS)
def test_the_next_eager_frame_uses_the_refreshed_winograd_filter(hip, cfg_reset, algo, mode):
    """One block, eagerly: after an in-place weight update the block's output is that of the new weights - bit-equal to the
    call that transforms the filter inside (no cached U) - and differs from the output before."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.nets.hip_modules import prepared_conv, set_net_mode
    algo(mode)
    net = build_net(18, DEV)
    set_net_mode('TEST')
    blk = net.resnet.layer1[1]
    x = torch.randn((1, 5, 7, 64), device=DEV)
    with torch.no_grad():
        before = blk(x).clone()
        assert ('_frcnn_winograd' in blk.conv2.__dict__) == (mode == 2)
        blk.conv2.weight.mul_(0.5)
        after = blk(x)
        w1, s1, b1 = prepared_conv(blk.conv1, blk.bn1)
        w2, s2, b2 = prepared_conv(blk.conv2, blk.bn2)
        mid = ops.conv2d_nhwc(x, w1, s1, b1, None, stride=1, pad=1, relu=True)
        want = ops.conv2d_nhwc_winograd_res(mid, w2, x, s2, b2, relu=True)
        torch.cuda.synchronize()
    assert torch.equal(after, want) and not torch.equal(after, before)
    if mode == 2:
        assert torch.equal(blk.conv2.__dict__['_frcnn_winograd'][1][0], ops.winograd_filter(w2))


@pytest.mark.gpu
def test_with_conv_bf16_a_block_is_the_composition_of_the_bf16_ops(hip, cfg_reset, algo, monkeypatch):
    """cfg.TEST.CONV_BF16 comes first in conv_forward, as for every inference convolution: an eligible block (C % 32 == 0) runs
    the existing bf16 form with its residual, bit for bit; the new entry point is not reached."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.nets.hip_modules import prepared_conv, set_net_mode
    cfg_reset.cfg.TEST.CONV_BF16 = True
    algo(2)
    calls = _winograd_res_calls(monkeypatch)
    net = build_net(18, DEV)
    set_net_mode('TEST')
    with torch.no_grad():
        for blk, c_in, hw in ((net.resnet.layer1[1], 64, (5, 7)), (net.resnet.layer2[0], 64, (6, 8)), (net.resnet.layer4[0], 256, (7, 7))):
            x = torch.randn((2,) + hw + (c_in,), device=DEV)
            got = blk(x)
            stride = blk.conv1.stride[0]
            w1, s1, b1 = prepared_conv(blk.conv1, blk.bn1)
            w2, s2, b2 = prepared_conv(blk.conv2, blk.bn2)
            identity = x
            if blk.downsample is not None:
                wd, sd, bd = prepared_conv(blk.downsample[0], blk.downsample[1])
                identity = ops.conv2d_nhwc_bf16(x, ops.conv2d_pack_bf16(wd), sd, bd, None, stride=stride, pad=0, relu=False)
            mid = ops.conv2d_nhwc_bf16(x, ops.conv2d_pack_bf16(w1), s1, b1, None, stride=stride, pad=1, relu=True)
            want = ops.conv2d_nhwc_bf16(mid, ops.conv2d_pack_bf16(w2), s2, b2, identity, stride=1, pad=1, relu=True)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
    assert calls == []
