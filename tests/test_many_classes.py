"""Detectors with more classes than the fused tail holds (K * (1 + E) > 64: more than 12 image classes, more than 8 LiDAR
classes) run their TEST-mode frames through the wide tail (ops.head_softmax_decode_wide, csrc/head.hip).  Before the wide form
existed every device test below raised HipError("head_fc_softmax_decode: bad shape ... classes ...") from the tail.

  image, 21 classes (PASCAL VOC)   256 x 320 ResNet-101 frame against O.ImageNetOracle(num_classes=21) on injected RPN logits:
                                   proposal indices, RoIs / cls_prob / bbox_pred within 1e-4, boxes by the rule of
                                   tests/test_gpu_parity._box_bounds_against_oracle, the per-class filter for all 20 foreground
                                   classes against O.filter_and_draw_prep; 81 classes (COCO): the tail and the filter alone on
                                   that frame's fc7
  LiDAR, 9 classes (KITTI's set)   208 x 176 BEV frame against O.LidarNetOracle(num_classes=9), stage by stage like
                                   test_lidar_detector_stagewise_against_oracle
  VGG16 / MobileNet, 21 classes    one TEST forward each against tests/vgg16_restatement.py / tests/mobilenet_restatement.py at
                                   the bars of tests/test_vgg16.py / tests/test_mobilenet.py
  captured frame                   a 21-class frame captured by FramePool and replayed twice equals the eager frame; a
                                   4-class detector of the same process still takes the fused kernel
  without a GPU                    the dispatch rule at 12 / 13 (image) and 8 / 9 (LiDAR) classes, and that Network._tail_kernel
                                   follows it
The oracle frames are evaluated once per process and shared.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import frcnn_oracle as O

DEV = "cuda:0"
_CACHE = {}


@pytest.fixture
def cfg_reset():
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    C.reset_cfg()
    try:
        yield C
    finally:
        C.reset_cfg()


def _ops():
    from faster_rcnn_pytorch_multimodal_amd import ops
    return ops


def _box_bounds(pred_boxes, pb_r, rois_r, what):
    """tests/test_gpu_parity._box_bounds_against_oracle: <= 1e-4 px where the box scale max(diagonal, |coordinate|) is
    <= 128 px, <= 12 ulp of that scale beyond."""
    rw, rh = rois_r[:, 3] - rois_r[:, 1] + 1.0, rois_r[:, 4] - rois_r[:, 2] + 1.0
    diag = torch.sqrt(rw * rw + rh * rh)
    diff = (pred_boxes - pb_r).abs()
    scale = torch.maximum(diag, pb_r.abs().max(1).values)
    ulp = torch.from_numpy(np.spacing(scale.numpy().astype(np.float32)))
    small = scale <= 128.0
    worst_small = float(diff[small].max()) if small.any() else 0.0
    worst_ulp = float((diff[~small] / ulp[~small, None]).max()) if (~small).any() else 0.0
    print("%s: |pred_boxes - reference| %.3e px on the %d boxes of scale <= 128 px, %.2f ulp(box scale) on the %d larger ones"
          % (what, worst_small, int(small.sum()), worst_ulp, int((~small).sum())))
    assert worst_small <= 1e-4, "%s: boxes up to 128 px differ by %.3e px" % (what, worst_small)
    assert worst_ulp <= 12.0, "%s: large boxes differ by %.2f ulp of their scale" % (what, worst_ulp)


def _centred_heads(sd, fc7, cls_std=2.0, box_std=0.5):
    """Head parameters that tell the RoIs apart, like a trained head's.  fc7 follows a ReLU and is dominated by one direction
    that all RoIs share, so a seeded head ranks the classes the same way for every RoI (one class takes them all).  Here the
    bias cancels the heads' response to the mean fc7 and the weights are scaled so that the logits spread by ``cls_std`` and
    the raw deltas by ``box_std`` over the RoIs.  Computed from the CPU oracle's fc7 only."""
    sd = dict(sd)
    fbar = fc7.double().mean(0)
    for name, target in (("cls_score_net", cls_std), ("bbox_pred_net", box_std)):
        w = sd[name + ".weight"].double()
        w = (w * (target / float(F.linear(fc7.double() - fbar, w).std()))).float()
        sd[name + ".weight"], sd[name + ".bias"] = w, (-(w.double() @ fbar)).float()
    return sd


def _oracle_frame(oracle, sd, data, info, structured, stds, means, decode):
    """oracle.test_frame with centred heads: the frame once (fc7 does not depend on the heads), then the oracle's own
    _region_classification and decode on its fc7, as its test_frame does."""
    oracle.load_state_dict(sd, strict=True)
    _, _, _, rois_r, _ = oracle.test_frame(data, info, structured)
    d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in oracle._dbg.items()}
    sd = _centred_heads(sd, d["fc7"])
    oracle.load_state_dict(sd, strict=True)
    k = oracle._num_classes
    with torch.no_grad():
        _, cp_r, bbox_pred = oracle._region_classification(d["fc7"])
    deltas = bbox_pred.mul(torch.tensor(stds).repeat(k).unsqueeze(0)).add(torch.tensor(means).repeat(k).unsqueeze(0))
    d["bbox_pred"] = bbox_pred
    return sd, cp_r, decode(rois_r, d, deltas), rois_r, d


def _to_device(net):
    net.eval()
    net._device = DEV
    net.to(DEV)
    return net


# ---- image, ResNet-101 -------------------------------------------------------------------------------------------------
IMG_H, IMG_W, IMG_THRESH, IMG_MAX_DETS = 256, 320, 0.1, 100
IMG_INFO = np.array([0, IMG_W, 0, IMG_H, 0, 0, 1.0], np.float32)


def _image_net(k, sd=None, seed=5):
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
    C.cfg.NET_TYPE = "image"
    if sd is None:
        sd = O.seeded_state_dict(O.ImageNetOracle(num_classes=k), seed, bn_mode="tame")
    net = imagenet(num_layers=101)
    net.create_architecture(k, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
    net.load_state_dict(sd, strict=True)
    return net, sd


def image21():
    """The 21-class oracle frame: evaluated once, never modified."""
    if "image21" not in _CACHE:
        import bench
        oracle = O.ImageNetOracle(num_classes=21)
        data = (np.random.default_rng(11).standard_normal((1, IMG_H, IMG_W, 3)) * 50).astype(np.float32)
        cls, box = bench.structured_rpn(7, IMG_H // 16, IMG_W // 16, 25)
        sd, cp_r, pb_r, rois_r, d = _oracle_frame(
            oracle, O.seeded_state_dict(oracle, 5, bn_mode="tame"), data, IMG_INFO, (cls, box), O.BBOX_NORMALIZE_STDS,
            O.BBOX_NORMALIZE_MEANS, lambda rois, d_, deltas: O.bbox_transform_inv(rois[:, 1:5], deltas, float(IMG_INFO[6])))
        _, boxes_r, _ = O.filter_and_draw_prep(rois_r, cp_r, pb_r, IMG_INFO, 21, IMG_THRESH)
        _CACHE["image21"] = dict(sd=sd, data=data, rpn=bench.fuse_rpn(cls, box), cp=cp_r, pb=pb_r, rois=rois_r, d=d,
                                 boxes=boxes_r)
    return _CACHE["image21"]


@pytest.mark.gpu
def test_image_detector_with_21_classes_against_oracle(hip, cfg_reset):
    from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device
    from faster_rcnn_pytorch_multimodal_amd.utils.filter_predictions import filter_and_draw_prep
    ops, ref = _ops(), image21()
    cp_r, pb_r, rois_r, d = ref["cp"], ref["pb"], ref["rois"], ref["d"]
    net = _to_device(_image_net(21, ref["sd"])[0])
    net._rpn_override = ref["rpn"].to(DEV)
    try:
        cs, cp, pb, rois, _ = net.test_frame(ref["data"], IMG_INFO)
        p = dict(net._predictions)
        fc7_dev = p["_tail"]["fc7"].clone()
        dets, counts = detect_frame_device(net, torch.from_numpy(ref["data"]).to(DEV), IMG_INFO, IMG_THRESH, IMG_MAX_DETS,
                                           IMG_MAX_DETS)
        dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    finally:
        net._rpn_override = None
    n = int(p["rois_count"].item())
    assert ops.head_uses_wide_form(21, 4)
    assert n == rois_r.shape[0] == rois.shape[0] and tuple(cp.shape) == (n, 21) and tuple(pb.shape) == (n, 84)
    assert torch.equal(p["rpn_order"][p["rpn_keep"][:n]].cpu(), d["order"][d["keep"]]), "proposal indices differ"
    np.testing.assert_allclose(rois.cpu().numpy(), rois_r.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(cp.cpu().numpy(), cp_r.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(p["bbox_pred"][:n].cpu().numpy(), d["bbox_pred"].numpy(), rtol=0, atol=1e-4)
    _box_bounds(pb.cpu(), pb_r, rois_r, "21 classes, composed frame")
    # the tail on the oracle's fc7 / rois
    with torch.no_grad():
        net._frame_scale = 1.0
        tail = net._tail_kernel(d["fc7"].contiguous().view(n, 1, 1, -1).to(DEV), rois_r.contiguous().to(DEV))
    np.testing.assert_allclose(tail["cls_prob"].cpu().numpy(), cp_r.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(tail["bbox_pred"].cpu().numpy(), d["bbox_pred"].numpy(), rtol=0, atol=1e-4)
    _box_bounds(tail["pred_boxes"].cpu(), pb_r, rois_r, "21 classes, tail on the oracle's fc7")
    # per-class filter, all 20 foreground classes: identical detections on the oracle's tensors, and the composed frame's
    # record against O.frame_detect (counts equal, scores within 1e-4, boxes within 1e-3 px)
    boxes_r = ref["boxes"]
    filled = [j for j in range(1, 21) if len(boxes_r[j])]
    print("21 classes: detections per class", [len(b) for b in boxes_r])
    assert len(filled) >= 15
    _, got_boxes, _ = filter_and_draw_prep(rois_r.to(DEV), cp_r.contiguous().to(DEV), pb_r.contiguous().to(DEV), {}, IMG_INFO,
                                           21, IMG_THRESH, "image")
    for j in range(1, 21):
        np.testing.assert_array_equal(np.asarray(got_boxes[j]).reshape(-1, 5), boxes_r[j])
        want = O.max_dets_cut(boxes_r[j], IMG_MAX_DETS)
        assert int(counts[j]) == len(want), "class %d: %d detections vs oracle %d" % (j, int(counts[j]), len(want))
        if len(want):
            g = dets[j, :len(want)]
            assert float(np.abs(g[:, 4] - want[:, 4]).max()) <= 1e-4 and float(np.abs(g[:, :4] - want[:, :4]).max()) <= 1e-3
    # ---- 81 classes: the tail and the filter alone, on this frame's fc7 -------------------------------------------------
    g = torch.Generator().manual_seed(81)
    stds, means = list(O.BBOX_NORMALIZE_STDS), list(O.BBOX_NORMALIZE_MEANS)
    f = fc7_dev[:n].contiguous()
    heads = _centred_heads({"cls_score_net.weight": torch.randn(81, 2048, generator=g),
                            "bbox_pred_net.weight": torch.randn(324, 2048, generator=g)}, f.cpu(), cls_std=3.0)
    wc, bc, wb, bb = (heads[m + e_] for m in ("cls_score_net", "bbox_pred_net") for e_ in (".weight", ".bias"))
    out = ops.head_softmax_decode_wide(f, wc.to(DEV), bc.to(DEV), wb.to(DEV), bb.to(DEV), rois[:n].contiguous(), stds, means, 1.0)
    f_cpu, rois_cpu = f.cpu(), rois[:n].cpu()
    cp81 = F.softmax(F.linear(f_cpu.double(), wc.double(), bc.double()), 1).float()
    bp81 = F.linear(f_cpu.double(), wb.double(), bb.double()).float()
    pb81 = O.bbox_transform_inv(rois_cpu[:, 1:5], bp81 * torch.tensor(stds).repeat(81) + torch.tensor(means).repeat(81), 1.0)
    np.testing.assert_allclose(out["cls_prob"].cpu().numpy(), cp81.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(out["bbox_pred"].cpu().numpy(), bp81.numpy(), rtol=0, atol=1e-4)
    _box_bounds(out["pred_boxes"].cpu(), pb81, rois_cpu, "81 classes, tail on the frame's fc7")
    thresh81 = 0.05
    _, boxes81, _ = O.filter_and_draw_prep(rois_cpu, cp81, pb81, IMG_INFO, 81, thresh81)
    print("81 classes: %d classes with detections, %d detections" % (sum(1 for b in boxes81 if len(b)), sum(len(b) for b in boxes81)))
    assert sum(1 for b in boxes81[1:] if len(b)) >= 40
    _, got81, _ = filter_and_draw_prep(rois_cpu.to(DEV), cp81.contiguous().to(DEV), pb81.contiguous().to(DEV), {}, IMG_INFO, 81,
                                       thresh81, "image")
    for j in range(1, 81):
        np.testing.assert_array_equal(np.asarray(got81[j]).reshape(-1, 5), boxes81[j])
    # and on the device's own tensors (probabilities a rounding away from the oracle's: a count may move by a box at the
    # threshold or at the NMS bar, so only the record's shape and the bulk of it are held)
    d81, c81 = ops.filter_per_class(out["pred_boxes"].clone(), out["cls_prob"], float(IMG_W), float(IMG_H), 1.0, thresh81,
                                    float(O.TEST_NMS_THRESH), n, n)
    want81 = np.array([len(b) for b in boxes81])
    assert tuple(d81.shape) == (81, n, 5) and int(c81[0]) == 0
    assert int(np.abs(c81.cpu().numpy()[1:] - want81[1:]).sum()) <= 2


# ---- LiDAR ---------------------------------------------------------------------------------------------------------------
BEV_H, BEV_W, LIDAR_THRESH = 208, 176, 0.15
LIDAR_INFO = np.array([0, BEV_W, 0, BEV_H, 0, 12, 0.5], np.float32)


@pytest.mark.gpu
def test_lidar_detector_with_9_classes_against_oracle(hip, cfg_reset):
    from faster_rcnn_pytorch_multimodal_amd.layer_utils.proposal_layer import proposal_layer
    from faster_rcnn_pytorch_multimodal_amd.nets.lidarnet import lidarnet
    from faster_rcnn_pytorch_multimodal_amd.utils.filter_predictions import filter_and_draw_prep
    C, ops, k = cfg_reset, _ops(), 9
    C.cfg.NET_TYPE = "lidar"
    oracle = O.LidarNetOracle(num_classes=k)
    rng = np.random.default_rng(3)
    data = (rng.random((1, BEV_H, BEV_W, 15)) * (rng.random((1, BEV_H, BEV_W, 15)) < 0.05)).astype(np.float32)
    sd, cp_r, pb_r, rois_r, d = _oracle_frame(
        oracle, O.seeded_state_dict(oracle, 9, bn_mode="tame"), data, LIDAR_INFO, None, O.LIDAR_BBOX_NORMALIZE_STDS,
        O.LIDAR_BBOX_NORMALIZE_MEANS,
        lambda rois, d_, deltas: O.lidar_3d_bbox_transform_inv(rois[:, 1:5], d_["roi_anchors_3d"], deltas, float(LIDAR_INFO[6])))
    net = lidarnet(num_layers=101)
    net.create_architecture(k, tag="default", anchor_scales=C.cfg.LIDAR.ANCHOR_SCALES[0], anchor_ratios=C.cfg.LIDAR.ANCHOR_ANGLES)
    net.load_state_dict(sd, strict=True)
    _to_device(net)
    # the composed frame runs (it raised before the wide tail) and its backbone agrees
    cs, cp, pb, rois, _ = net.test_frame(data, LIDAR_INFO)
    assert ops.head_uses_wide_form(k, 7)
    assert tuple(cp.shape) == (rois.shape[0], k) and tuple(pb.shape) == (rois.shape[0], 7 * k)
    assert bool(torch.isfinite(cp).all()) and bool(torch.isfinite(pb).all())
    conv, conv_r = net._act_summaries["conv"].cpu().permute(0, 3, 1, 2).numpy(), d["net_conv"].numpy()
    assert float(np.abs(conv - conv_r).max()) <= 5e-5 * float(np.abs(conv_r).max())
    # proposals on the oracle's probabilities / deltas
    blob, scores, a3 = proposal_layer(d["rpn_cls_prob"].to(DEV), d["rpn_bbox_pred"].to(DEV), LIDAR_INFO, "TEST",
                                      d["anchors"].to(DEV), d["anchors_3d"].to(DEV), oracle._num_anchors)
    assert blob.shape[0] == rois_r.shape[0]
    np.testing.assert_allclose(blob.cpu().numpy(), rois_r.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_array_equal(a3.cpu().numpy(), d["roi_anchors_3d"].numpy())
    # tail on the oracle's pooled features / rois / anchors (P = 7: the wide form takes the spatial mean first)
    with torch.no_grad():
        y = net.resnet.layer4(d["pool5"].permute(0, 2, 3, 1).contiguous().to(DEV))
        net._frame_scale = 0.5
        net._predictions["roi_anchors_3d"] = d["roi_anchors_3d"].contiguous().to(DEV)
        tail = net._tail_kernel(y, rois_r.contiguous().to(DEV))
    fc7, fc7_r = tail["fc7"].cpu().numpy(), d["fc7"].numpy()
    assert float(np.abs(fc7 - fc7_r).max()) <= 5e-5 * float(np.abs(fc7_r).max())
    np.testing.assert_allclose(tail["cls_prob"].cpu().numpy(), cp_r.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(tail["bbox_pred"].cpu().numpy(), d["bbox_pred"].numpy(), rtol=0, atol=1e-4)
    own = O.lidar_3d_bbox_transform_inv(rois_r[:, 1:5], d["roi_anchors_3d"],
                                        tail["bbox_pred"].cpu() * torch.tensor(O.LIDAR_BBOX_NORMALIZE_STDS).repeat(k)
                                        + torch.tensor(O.LIDAR_BBOX_NORMALIZE_MEANS).repeat(k), 0.5)
    np.testing.assert_allclose(tail["pred_boxes"].cpu().numpy(), own.numpy(), rtol=3e-7, atol=1e-4)
    np.testing.assert_allclose(tail["pred_boxes"].cpu().numpy(), pb_r.numpy(), rtol=1e-4, atol=2e-3)
    # per-class filter on the oracle's probabilities / boxes: identical detections for all 8 foreground classes
    _, ref_boxes = O.filter_and_draw_prep_lidar(rois_r, cp_r, pb_r, k, thresh=LIDAR_THRESH)
    print("9 LiDAR classes: detections per class", [len(b) for b in ref_boxes])
    assert all(len(b) for b in ref_boxes[1:])
    _, got_boxes, _ = filter_and_draw_prep(rois_r.to(DEV), cp_r.contiguous().to(DEV), pb_r.contiguous().to(DEV), {}, LIDAR_INFO,
                                           k, LIDAR_THRESH, "lidar")
    for j in range(1, k):
        np.testing.assert_array_equal(np.asarray(got_boxes[j]).reshape(-1, 8), ref_boxes[j])


# ---- VGG16 and MobileNet -----------------------------------------------------------------------------------------------
def _heads_on_own_fc7(net, p, n, k, what):
    """The heads on the device's own fc7 (the bars of tests/test_vgg16.py / tests/test_mobilenet.py: 1e-4), the decoded boxes
    by the box rule against the CPU decode of the CPU heads."""
    f = p["_tail"]["fc7"][:n].cpu()
    with torch.no_grad():
        score = F.linear(f, net.cls_score_net.weight.cpu(), net.cls_score_net.bias.cpu())
        raw = F.linear(f, net.bbox_pred_net.weight.cpu(), net.bbox_pred_net.bias.cpu())
    assert tuple(p["cls_prob"].shape[1:]) == (k,) and tuple(p["pred_boxes"].shape[1:]) == (4 * k,)
    np.testing.assert_allclose(p["cls_score"][:n].cpu().numpy(), score.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(p["cls_prob"][:n].cpu().numpy(), F.softmax(score, 1).numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(p["bbox_pred"][:n].cpu().numpy(), raw.numpy(), rtol=0, atol=1e-4)
    rois = p["rois"][:n].cpu()
    deltas = raw * torch.tensor(O.BBOX_NORMALIZE_STDS).repeat(k) + torch.tensor(O.BBOX_NORMALIZE_MEANS).repeat(k)
    _box_bounds(p["pred_boxes"][:n].cpu(), O.bbox_transform_inv(rois[:, 1:5], deltas, 1.0), rois, what)


@pytest.mark.gpu
def test_vgg16_with_21_classes(hip, cfg_reset):
    import test_vgg16 as TV
    from faster_rcnn_pytorch_multimodal_amd.nets.vgg16 import vgg16
    C = cfg_reset
    C.cfg.NET_TYPE = "image"
    C.cfg.TEST.RPN_POST_NMS_TOP_N = 50
    torch.manual_seed(3)
    net = vgg16()
    net.create_architecture(21, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
    net.vgg.load_state_dict(TV.state(), strict=True)
    _to_device(net)
    blob = TV._frame(np.random.default_rng(1))
    with torch.no_grad():
        rois, cls_prob, bbox_pred = net.forward(blob, TV.INFO, None, None, mode="TEST")
        p = dict(net._predictions)
        n = int(p["rois_count"].item())
        assert 0 < n <= 50 and tuple(cls_prob.shape) == (50, 21) and tuple(bbox_pred.shape) == (50, 84)
        net_conv = net._act_summaries["conv"]
        s64, e32 = TV.restated(TV.R.head, blob.transpose(0, 3, 1, 2))
        err = float(np.abs(net_conv.permute(0, 3, 1, 2).cpu().numpy().astype(np.float64) - s64[-1]).max())
        assert err <= 8 * e32[-1]
        pool5 = net._crop_pool_layer(net_conv.permute(0, 3, 1, 2), rois)
        fc7 = net._head_to_tail(pool5)
        assert tuple(fc7.shape) == (50, 4096) and torch.equal(fc7, p["_tail"]["fc7"])
        t64, e32t = TV.restated(TV.R.tail, pool5[:n].cpu().numpy())
        err = float(np.abs(fc7[:n].cpu().numpy().astype(np.float64) - t64[-1]).max())
        assert err <= 8 * e32t[-1]
    _heads_on_own_fc7(net, p, n, 21, "VGG16, 21 classes")


@pytest.mark.gpu
def test_mobilenet_with_21_classes(hip, cfg_reset):
    import test_mobilenet as TM
    from faster_rcnn_pytorch_multimodal_amd.nets.mobilenet_v1 import mobilenetv1
    C = cfg_reset
    C.cfg.NET_TYPE = "image"
    C.cfg.TEST.RPN_POST_NMS_TOP_N = 50
    torch.manual_seed(3)
    net = mobilenetv1()
    net.create_architecture(21, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
    net.mobilenet.load_state_dict(TM.states()[1], strict=True)
    _to_device(net)
    blob = TM._frame(np.random.default_rng(1))
    with torch.no_grad():
        rois, cls_prob, bbox_pred = net.forward(blob, TM.INFO, None, None, mode="TEST")
        p = dict(net._predictions)
        n = int(p["rois_count"].item())
        assert 0 < n <= 50 and tuple(cls_prob.shape) == (50, 21) and tuple(bbox_pred.shape) == (50, 84)
        net_conv = net._act_summaries["conv"]
        y64, e32 = TM.restated(TM.R.head, blob.transpose(0, 3, 1, 2))
        err = float(np.abs(net_conv.permute(0, 3, 1, 2).cpu().numpy().astype(np.float64) - y64).max())
        assert err <= 8 * e32
        pool5 = net._crop_pool_layer(net_conv.permute(0, 3, 1, 2), rois)
        fc7 = net._head_to_tail(pool5)
        assert fc7.shape[1] == 1024 and torch.equal(fc7, p["_tail"]["fc7"])
        t64, e32t = TM.restated(TM.R.tail, pool5[:n].cpu().numpy())
        err = float(np.abs(fc7[:n].cpu().numpy().astype(np.float64) - t64).max())
        assert err <= 8 * e32t
    _heads_on_own_fc7(net, p, n, 21, "MobileNet, 21 classes")


# ---- captured frames ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_21_class_frame_and_the_fused_kernel_beside_it(hip, cfg_reset, monkeypatch):
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FramePool
    from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device
    ops, ref = _ops(), image21()
    calls = {"wide": 0, "fused": 0}

    def counted(name, fn):
        def inner(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return inner
    monkeypatch.setattr(ops, "head_softmax_decode_wide", counted("wide", getattr(ops, "head_softmax_decode_wide", None)),
                        raising=False)
    monkeypatch.setattr(ops, "head_fc_softmax_decode", counted("fused", ops.head_fc_softmax_decode))
    net = _to_device(_image_net(21, ref["sd"])[0])
    data = torch.from_numpy(ref["data"]).to(DEV)
    with torch.no_grad():
        dets, counts = detect_frame_device(net, data, IMG_INFO, IMG_THRESH, IMG_MAX_DETS, IMG_MAX_DETS)
    dets, counts = dets.clone(), counts.clone()
    torch.cuda.synchronize()
    assert calls == {"wide": 1, "fused": 0} and int(counts[1:].sum()) > 0
    pool = FramePool(net, streams=1, capture_after=1, autotune=False)
    runner = pool.runner((1, IMG_H, IMG_W, 3), IMG_INFO, IMG_THRESH, IMG_MAX_DETS)
    assert runner is not None and runner.graph is not None and pool.stats["captures"] == 1 and not pool.uncapturable
    for _ in range(2):
        g_d, g_c = runner.run(data, poison=True)
        torch.cuda.synchronize()
        assert torch.equal(g_c, counts) and torch.equal(g_d, dets)
    # the tail by itself under torch's synchronisation check, and captured: neither launch waits for the host
    p = runner.predictions
    n = int(p["rois_count"].item())
    args = (p["_tail"]["fc7"].clone(), net.cls_score_net.weight.detach(), net.cls_score_net.bias.detach(),
            net.bbox_pred_net.weight.detach(), net.bbox_pred_net.bias.detach(), p["rois"].clone(),
            list(O.BBOX_NORMALIZE_STDS), list(O.BBOX_NORMALIZE_MEANS), 1.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = ops.head_softmax_decode_wide(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for name in ("cls_score", "cls_prob", "bbox_pred"):          # the frame's pred_boxes were clamped in place by its filter
        assert torch.equal(eager[name][:n], p[name][:n]), name
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = ops.head_softmax_decode_wide(*args)
    for _ in range(2):
        for name in ("cls_prob", "pred_boxes"):
            held[name].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for name in ("cls_score", "cls_prob", "bbox_pred", "pred_boxes"):
            assert torch.equal(held[name], eager[name]), name
    # a 4-class detector in the same process: the rule keeps the fused kernel, and its results are that kernel's bits
    before = dict(calls)
    assert not ops.head_uses_wide_form(4, 4)
    net4 = _to_device(_image_net(4)[0])
    with torch.no_grad():
        net4.forward(data, IMG_INFO, None, None, mode="TEST")
    q = net4._predictions
    assert calls["wide"] == before["wide"] and calls["fused"] == before["fused"] + 1
    r, c = q["_tail"]["fc7"].shape
    direct = ops.head_fc_softmax_decode(q["_tail"]["fc7"].view(r, 1, 1, c), net4.cls_score_net.weight.detach(),
                                        net4.cls_score_net.bias.detach(), net4.bbox_pred_net.weight.detach(),
                                        net4.bbox_pred_net.bias.detach(), q["rois"].contiguous(), list(O.BBOX_NORMALIZE_STDS),
                                        list(O.BBOX_NORMALIZE_MEANS), 1.0)
    for name in ("cls_score", "cls_prob", "bbox_pred", "pred_boxes"):
        assert torch.equal(direct[name], q[name]), name


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_dispatch_rule_at_the_fused_kernels_limits():
    ops = _ops()
    assert ops.HEAD_FUSED_MAX_OUT == 64
    assert [ops.head_uses_wide_form(k, 4) for k in (2, 12, 13, 21, 81)] == [False, False, True, True, True]
    assert [ops.head_uses_wide_form(k, 7) for k in (2, 8, 9, 11)] == [False, False, True, True]


@pytest.mark.parametrize("net_type,k,wide", [("image", 12, False), ("image", 13, True), ("lidar", 8, False), ("lidar", 9, True)])
def test_tail_kernel_follows_the_dispatch_rule(cfg_reset, monkeypatch, net_type, k, wide):
    """Network._tail_kernel with both ops replaced by recorders (no device): which one is called, and with what."""
    from faster_rcnn_pytorch_multimodal_amd.nets import network as N
    C = cfg_reset
    C.cfg.NET_TYPE = net_type
    e = 7 if net_type == "lidar" else 4
    seen = []
    monkeypatch.setattr(N.ops, "head_softmax_decode_wide", lambda fc7, *a, **kw: seen.append(("wide", tuple(fc7.shape), kw)) or {})
    monkeypatch.setattr(N.ops, "head_fc_softmax_decode", lambda x, *a, **kw: seen.append(("fused", tuple(x.shape), kw)) or {})

    class Stub(object):
        cls_score_net = torch.nn.Linear(8, k)
        bbox_pred_net = torch.nn.Linear(8, e * k)
        _frame_scale = 1.0
        _predictions = {"roi_anchors_3d": torch.zeros(3, 7)}
    N.Network._tail_kernel(Stub(), torch.zeros(3, 1, 1, 8), torch.zeros(3, 5))
    assert len(seen) == 1
    name, shape, kw = seen[0]
    assert name == ("wide" if wide else "fused") and shape == ((3, 8) if wide else (3, 1, 1, 8))
    assert (kw["roi_anchors_3d"] is not None) == (net_type == "lidar")
