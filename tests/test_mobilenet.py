"""nets.mobilenet_v1.mobilenetv1 (the reference's ``--net mobile`` detector, inference).

References: tests/golden/mobilenet_v1.npz (written by tests/golden/make_golden_mobilenet.py from the reference's own
modules: key / shape list, weight checksums, an input with the head's output, a pooled input with the tail's output) and
tests/mobilenet_restatement.py (the body restated with torch functional calls, run in fp32 and float64; weights come
from names, shapes and a seed on both sides).

Bounds.  e32 = max |restatement fp32 - restatement float64| on the tensors of the check is the error an fp32 evaluation
of this function has on this input.  The golden outputs are another fp32 evaluation (another summation order): 4 * e32.
The device sums the same fp32 products in MFMA / split-bf16 order: 8 * e32.  A wrong tap, stride, pad or clamp site is an
error of order 0.1 - 1.
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import mobilenet_restatement as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "faster_rcnn_pytorch_multimodal_amd", "compat")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mobilenet_v1.npz")
DEV = "cuda:0"
_CACHE = {}


def golden():
    if "g" not in _CACHE:
        g = np.load(GOLDEN)
        shapes = [(str(k), tuple(int(v) for v in s.split(",") if v)) for k, s in zip(g["keys"], g["shapes"])]
        _CACHE["g"] = dict(shapes=shapes, checksums=g["checksums"], seed=int(g["seed"]), x=g["x"], head_out=g["head_out"],
                           pooled=g["pooled"], tail_out=g["tail_out"])
    return _CACHE["g"]


def states():
    """The seeded weights as (numpy float64, torch fp32, torch float64) - made once, never modified."""
    if "s" not in _CACHE:
        import torch
        g = golden()
        st = R.seeded_state(g["shapes"], g["seed"])
        _CACHE["s"] = (st, R.torch_state(st, torch.float32), R.torch_state(st, torch.float64))
    return _CACHE["s"]


def restated(fn, x):
    """(float64 result, e32) of ``fn`` = R.head / R.tail on the NCHW numpy array ``x``."""
    import torch
    _, s32, s64 = states()
    with torch.no_grad():
        y64 = fn(s64, torch.from_numpy(np.asarray(x, np.float64))).numpy()
        y32 = fn(s32, torch.from_numpy(np.asarray(x, np.float32))).numpy()
    return y64, float(np.abs(y32.astype(np.float64) - y64).max())


def build_net(device=None, seed=3):
    import torch
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.nets.mobilenet_v1 import mobilenetv1
    torch.manual_seed(seed)
    net = mobilenetv1()
    net.create_architecture(2, tag='default', anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
    net.mobilenet.load_state_dict(states()[1], strict=True)
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
def test_state_dict_has_the_reference_keys(cfg_reset):
    from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
    net = build_net()
    sd = net.state_dict()
    body = [(k[len("mobilenet."):], tuple(v.shape)) for k, v in sd.items() if k.startswith("mobilenet.")]
    assert body == golden()["shapes"] and len(body) == 27 * 6
    res = imagenet(num_layers=50)
    res.create_architecture(2, tag='default')
    assert [k for k in sd if not k.startswith("mobilenet.")] == [k for k in res.state_dict() if not k.startswith("resnet.")]
    assert tuple(sd["rpn_net.weight"].shape) == (512, 512, 3, 3) and tuple(sd["cls_score_net.weight"].shape) == (2, 1024)
    assert tuple(sd["bbox_pred_net.weight"].shape) == (8, 1024)
    assert (net._feat_stride, net._net_conv_channels, net._fc7_channels, net._det_net_channels,
            net._roi_pooling_channels) == (16, 512, 1024, 1024, 512)
    assert len(list(net._layers['head'])) == 12 and len(list(net._layers['tail'])) == 2
    # load_pretrained_cnn (mobilenet_v1.py:289-293): the body's keys under 'features.', anything else is ignored
    other = {"features." + k: v + 1 for k, v in states()[1].items()}
    other["classifier.weight"] = other["features.Conv2d_0.0.weight"]
    net.load_pretrained_cnn(other)
    got = net.mobilenet.state_dict()
    assert all((got[k] == states()[1][k] + 1).all() for k in got)


def test_reference_import_line_gives_the_package_class(tmp_path):
    script = textwrap.dedent("""
        import sys
        sys.path = [p for p in sys.path if p not in ('', %(root)r)]
        sys.path.insert(0, %(compat)r)
        from nets.mobilenet_v1 import mobilenetv1
        from nets.network import Network
        from model.config import cfg, cfg_from_list
        import faster_rcnn_pytorch_multimodal_amd.nets.mobilenet_v1 as real
        assert mobilenetv1 is real.mobilenetv1 and issubclass(mobilenetv1, Network)
        assert cfg.MOBILENET == dict(REGU_DEPTH=False, FIXED_LAYERS=5, WEIGHT_DECAY=0.00004, DEPTH_MULTIPLIER=1.0)
        cfg_from_list(['NET_TYPE', 'image'])              # tools/test_net.py: the image detector's CLI value
        net = mobilenetv1()
        net.create_architecture(2, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
        assert 'mobilenet.Conv2d_3.depthwise.1.running_var' in net.state_dict()
        print('mobile ok')
    """) % {"root": ROOT, "compat": COMPAT}
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    out = subprocess.run([sys.executable, "-c", script], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert out.returncode == 0 and "mobile ok" in out.stdout, out.stderr[-3000:]


@pytest.mark.parametrize("fixed,regu", [(5, False), (0, True), (12, False)])
def test_freezing_and_weight_decay_follow_the_config(cfg_reset, fixed, regu):
    import torch.nn as nn
    cfg = cfg_reset.cfg
    cfg.MOBILENET.FIXED_LAYERS, cfg.MOBILENET.REGU_DEPTH = fixed, regu
    net = build_net()
    for i, child in enumerate(net.mobilenet.children()):
        for m in child.modules():
            if isinstance(m, nn.BatchNorm2d):
                assert not m.weight.requires_grad and not m.bias.requires_grad
            elif isinstance(m, nn.Conv2d):
                assert m.weight.requires_grad == (i >= fixed), i
                assert m.weight.weight_decay == (cfg.MOBILENET.WEIGHT_DECAY if (regu or m.groups == 1) else 0)
    assert all(p.requires_grad for n, p in net.named_parameters() if not n.startswith("mobilenet."))


def test_train_keeps_batchnorm_and_fixed_layers_in_eval_mode(cfg_reset):
    import torch.nn as nn
    net = build_net()
    assert net.train() is net and net.training
    children = list(net.mobilenet.children())
    assert all(not m.training for c in children[:5] for m in c.modules())
    assert all(m.training for c in children[5:] for m in c.modules() if isinstance(m, nn.Conv2d))
    assert all(not m.training for m in net.mobilenet.modules() if isinstance(m, nn.BatchNorm2d))
    assert net.rpn_net.training
    net.eval()
    assert not any(m.training for m in net.modules())


def test_what_is_not_built_raises(cfg_reset):
    from faster_rcnn_pytorch_multimodal_amd.nets.mobilenet_v1 import mobilenetv1
    cfg = cfg_reset.cfg
    net = build_net()
    blob, info = np.zeros((1, 32, 32, 3), np.float32), np.array([0, 32, 0, 32, 0, 0, 1.0], np.float32)
    with pytest.raises(NotImplementedError, match="inference only"):
        net.forward(blob, info, np.zeros((1, 5), np.float32), None, mode='TRAIN')
    with pytest.raises(NotImplementedError, match="inference only"):
        net(blob, info, np.zeros((1, 5), np.float32))                      # the default mode is TRAIN
    for set_flag in (lambda: cfg.MOBILENET.__setitem__('DEPTH_MULTIPLIER', 0.5), lambda: setattr(cfg, 'ENABLE_CUSTOM_TAIL', True),
                     lambda: setattr(cfg, 'USE_FPN', True), lambda: cfg.UC.__setitem__('EN_BBOX_ALEATORIC', True),
                     lambda: cfg.UC.__setitem__('EN_CLS_EPISTEMIC', True), lambda: cfg.UC.__setitem__('EN_RPN_CLS_ALEATORIC', True)):
        cfg_reset.reset_cfg()
        cfg.NET_TYPE = "image"
        set_flag()
        with pytest.raises(NotImplementedError):
            mobilenetv1()
    cfg_reset.reset_cfg()
    mobilenetv1()


def test_regenerated_weights_match_the_checksums():
    g = golden()
    assert [k for k, _ in g["shapes"]] == [k for k, _ in R.key_shapes()] and g["shapes"] == R.key_shapes()
    sums = R.checksums(states()[0])
    got = np.array([sums[k] for k, _ in g["shapes"]])
    np.testing.assert_allclose(got, g["checksums"], rtol=1e-12, atol=0)


def test_restatement_agrees_with_the_reference_outputs():
    g = golden()
    for fn, x, want in ((R.head, g["x"], g["head_out"]), (R.tail, g["pooled"], g["tail_out"])):
        y64, e32 = restated(fn, x)
        gap = float(np.abs(want.astype(np.float64) - y64).max())
        print("%s: e32 %.3g, |golden - float64| %.3g (%.2f e32)" % (fn.__name__, e32, gap, gap / e32))
        assert want.shape == y64.shape and 0 < e32 < 1e-3
        assert gap <= 4 * e32


def test_no_stage_dies_or_saturates():
    import torch
    g = golden()
    s64 = states()[2]
    stages = []
    with torch.no_grad():
        R.head(s64, torch.from_numpy(g["x"]).double(), stages)
        R.tail(s64, torch.from_numpy(g["pooled"]).double(), stages)
    assert len(stages) == 14
    for i, s in enumerate(stages):
        assert float(((s > 0) & (s < 6)).double().mean()) >= 0.25, i
    assert int((stages[11] == 6).sum()) >= 1 and int((stages[13] == 6).sum()) >= 1      # net_conv and Conv2d_13 clamp


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _frame(rng, h=160, w=256):
    return (rng.standard_normal((1, h, w, 3)) * 1.0).astype(np.float32)


INFO = np.array([0, 256, 0, 160, 0, 0, 1.0], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("split_bf16", [True, False])
def test_head_and_tail_against_float64(hip, cfg_reset, split_bf16):
    """``_image_to_head`` on the golden input and ``_head_to_tail`` on the golden pooled input: max |device - float64| <=
    8 * e32.  Measured ratios are recorded in profiles/mobilenet.md."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.nets.hip_modules import set_net_mode, to_nchw_view
    cfg_reset.cfg.TEST.CONV_SPLIT_BF16 = split_bf16
    g = golden()
    net = build_net(DEV)
    net._mode = 'TEST'
    set_net_mode('TEST')
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(g["x"].transpose(0, 2, 3, 1))).to(DEV)
        net._image = to_nchw_view(ops.pad_channels(x, 4))
        net_conv = net._image_to_head()
        assert tuple(net_conv.shape) == (1, 512, 4, 6) and net._act_summaries['conv'].is_contiguous()
        net._predictions = {'rois': torch.zeros((2, 5), device=DEV)}
        pooled = torch.from_numpy(g["pooled"]).to(DEV)
        fc7 = net._head_to_tail(pooled)
        assert tuple(fc7.shape) == (2, 1024) and net._predictions['_tail']['fc7'] is fc7
        torch.cuda.synchronize()
    for name, fn, x_np, got in (("net_conv", R.head, g["x"], net_conv.cpu().numpy()), ("fc7", R.tail, g["pooled"], fc7.cpu().numpy())):
        y64, e32 = restated(fn, x_np)
        err = float(np.abs(got.astype(np.float64) - y64).max())
        print("mobilenet %s (split_bf16=%s): max |device - float64| %.3g = %.2f e32 (e32 %.3g)" % (name, split_bf16, err, err / e32, e32))
        assert err <= 8 * e32, (name, err, e32)
    assert float(net_conv.max()) == 6.0 and float(net_conv.min()) == 0.0


def _eager(net, blob, info):
    import torch
    with torch.no_grad():
        net.forward(blob, info, None, None, mode='TEST')
    torch.cuda.synchronize()
    p = net._predictions
    return {k: p[k].clone() for k in ('rois', 'rois_count', 'cls_score', 'cls_prob', 'bbox_pred', 'pred_boxes')}


@pytest.mark.gpu
def test_whole_frame_stage_by_stage(hip, cfg_reset):
    """forward(mode='TEST') and test_frame on a 160x256 frame; every stage is checked on the device's own input tensors."""
    import torch
    import torch.nn.functional as F
    cfg_reset.cfg.TEST.RPN_POST_NMS_TOP_N = 50
    net = build_net(DEV)
    blob = _frame(np.random.default_rng(1))
    with torch.no_grad():
        rois, cls_prob, bbox_pred = net.forward(blob, INFO, None, None, mode='TEST')
        p = dict(net._predictions)
        n = int(p['rois_count'].item())
        assert 0 < n <= 50 and tuple(rois.shape) == (50, 5)
        assert tuple(cls_prob.shape) == (50, 2) and tuple(bbox_pred.shape) == (50, 8) and tuple(p['pred_boxes'].shape) == (50, 8)
        # net_conv against the restatement
        net_conv = net._act_summaries['conv']
        assert tuple(net_conv.shape) == (1, 10, 16, 512)
        y64, e32 = restated(R.head, blob.transpose(0, 3, 1, 2))
        err = float(np.abs(net_conv.permute(0, 3, 1, 2).cpu().numpy().astype(np.float64) - y64).max())
        print("frame net_conv: %.3g = %.2f e32" % (err, err / e32))
        assert err <= 8 * e32
        # the tail on the device's own pool5
        fc7_frame = p['_tail']['fc7']
        pool5 = net._crop_pool_layer(net_conv.permute(0, 3, 1, 2), rois)
        assert tuple(pool5.shape) == (50, 512, 7, 7)
        fc7 = net._head_to_tail(pool5)
        assert torch.equal(fc7, fc7_frame)
        t64, e32t = restated(R.tail, pool5[:n].cpu().numpy())
        err = float(np.abs(fc7[:n].cpu().numpy().astype(np.float64) - t64).max())
        print("frame fc7: %.3g = %.2f e32" % (err, err / e32t))
        assert err <= 8 * e32t
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


@pytest.mark.gpu
def test_captured_frame_replays_and_follows_new_weights(hip, cfg_reset):
    import torch
    cfg_reset.cfg.TEST.RPN_POST_NMS_TOP_N = 50
    net = build_net(DEV)
    rng = np.random.default_rng(2)
    frames = [_frame(rng), _frame(rng)]
    net.enable_frame_graphs()
    pool = net.frame_pool(streams=1, autotune=False)
    runner = pool.runner(frames[0].shape, INFO, with_filter=False)
    assert runner is not None and runner.graph is not None and pool.stats['captures'] == 1
    keys = ('rois', 'rois_count', 'cls_score', 'cls_prob', 'bbox_pred', 'pred_boxes')

    def replay(frame):
        for k in keys:                                      # poison: a replay that did not run leaves no plausible result
            runner.predictions[k].fill_(-7 if runner.predictions[k].dtype != torch.float32 else float('nan'))
        runner.run(frame)
        torch.cuda.synchronize()
        return {k: runner.predictions[k].clone() for k in keys}

    def check_equal(a, b):
        for k in keys:
            assert torch.equal(a[k], b[k]), k

    eager = [_eager(net, f, INFO) for f in frames]
    assert int(eager[0]['rois_count']) > 0 and not torch.equal(eager[0]['cls_prob'], eager[1]['cls_prob'])
    for _ in range(2):
        for f, e in zip(frames, eager):
            check_equal(replay(f), e)
    # the same graph after an in-place weight change: prepared_depthwise's refresh hook re-derives the tensors it reads
    dw, pw = net.mobilenet.Conv2d_4.depthwise[0], net.mobilenet.Conv2d_12.pointwise[0]
    ptr = dw.__dict__['_frcnn_prepared_dw'][1][0].data_ptr()
    with torch.no_grad():
        dw.weight.mul_(1.01)
        net.mobilenet.Conv2d_13.depthwise[0].weight.mul_(1.01)
        pw.weight.mul_(1.01)
    pool.sync_weights()
    assert pool.stats['refreshes'] == 1 and pool.stats['invalidations'] == 0 and pool.stats['captures'] == 1
    assert dw.__dict__['_frcnn_prepared_dw'][1][0].data_ptr() == ptr
    assert torch.equal(dw.__dict__['_frcnn_prepared_dw'][1][0], dw.weight.detach().reshape(-1, 3, 3).permute(1, 2, 0))
    after = replay(frames[0])
    assert not torch.equal(after['cls_score'], eager[0]['cls_score'])
    check_equal(after, _eager(net, frames[0], INFO))
    # test_frame goes through the same pool
    out = net.test_frame(frames[0], INFO)
    n = int(after['rois_count'])
    assert torch.equal(out[1], after['cls_prob'][:n]) and pool.stats['captures'] == 1


class _RefDb:
    """lib/datasets/db.py:39-40,46-51,139-148 - the members lib/model/test.py reads."""
    name = "synthetic_db"
    num_classes = 2

    def __init__(self, directory, files):
        self._dir, self._val_index, self._test_index = directory, list(files), []
        self.evaluated = None

    def path_at(self, i, mode="train"):
        return os.path.join(self._dir, mode, self._val_index[i]) if mode == "val" else None

    def evaluate_detections(self, all_boxes, output_dir, mode):
        self.evaluated = (len(all_boxes), output_dir, mode)


@pytest.mark.gpu
def test_test_net_over_three_frames(hip, cfg_reset, tmp_path):
    """model.test.test_net (lib/model/test.py:138-257) with the reference's db protocol: all_boxes[cls][frame] rows of
    [x1, y1, x2, y2, score], equal to the eager per-frame path."""
    import torch
    import faster_rcnn_pytorch_multimodal_amd.model.test as T
    cfg = cfg_reset.cfg
    cfg.TEST.RPN_POST_NMS_TOP_N = 50
    cfg.TEST.GRAPH_AUTOTUNE = False
    cfg.ROOT_DIR = str(tmp_path)
    os.makedirs(tmp_path / "val")
    rng = np.random.default_rng(4)
    files = []
    for i in range(3):
        files.append("frame_%d.npy" % i)
        np.save(tmp_path / "val" / files[-1], rng.integers(0, 256, (160, 256, 3), dtype=np.uint8))
    db = _RefDb(str(tmp_path), files)
    net = build_net(DEV)
    timers = {}
    all_boxes = T.test_net(net, db, None, max_dets=100, mode='val', thresh=0.05, draw_det=False, eval_det=True, timers=timers)
    assert db.evaluated is not None and db.evaluated[0] == 2 and db.evaluated[2] == 'val'
    assert len(all_boxes) == 2 and all(len(per_class) == 3 for per_class in all_boxes)
    assert timers["pool"]["replays"] == 3 and timers["pool"]["eager"] == 0, timers
    total = 0
    for i in range(3):
        blobs = T._get_blobs([db.path_at(i, "val")])
        dets, counts = T.detect_frame_device(net, blobs["data"], blobs["info"], 0.05, 100, 100)
        torch.cuda.synchronize()
        assert all_boxes[0][i].size == 0                                  # the background class has no rows
        k = int(counts[1])
        got = all_boxes[1][i].reshape(-1, 5)
        assert got.shape[0] == k
        np.testing.assert_array_equal(got, dets[1, :k].cpu().numpy())
        total += k
    assert total > 0
