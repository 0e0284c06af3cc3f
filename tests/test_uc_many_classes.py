"""Uncertainty heads (cfg.UC.*) on detectors with more than 16 classes: the training step's Bayesian cross entropy through
frcnn_bayesian_cross_entropy_wide, and the per-detection uncertainty columns of a 21-class TEST frame.

Frames: 160 x 224 images and the 208 x 176 BEV frame of tests/test_uncertainty.py.  Bars are that file's: 5e-5 on the
classification loss against O.bayesian_cross_entropy on the step's own cls_score / cls_var and seed; 2e-6 * max(1, max |ref|)
on the loss's gradients with respect to the two class heads' outputs; on the heads' parameter gradients (X^T d against float64
autograd through O.UcHeadsOracle) that bar times sum_n |x| plus 2e-5 * max(1, max |ref|) for the fp32 GEMM; rtol 1e-4 / atol
2e-5 * max(1, max |ref|) on the uncertainty terms.
"""
import warnings

import numpy as np
import pytest
import torch

from oracle import frcnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AL = dict(EN_BBOX_ALEATORIC=True, EN_CLS_ALEATORIC=True)
ALL_FLAGS = dict(EN_BBOX_EPISTEMIC=True, EN_CLS_EPISTEMIC=True, EN_BBOX_ALEATORIC=True, EN_CLS_ALEATORIC=True)
CLS_AL = dict(EN_CLS_ALEATORIC=True)
IMG_H, IMG_W = 160, 224
IMG_INFO = np.array([0, IMG_W, 0, IMG_H, 0, 0, 1.0], np.float32)


@pytest.fixture
def cfg_reset():
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    C.reset_cfg()
    try:
        yield C
    finally:
        C.reset_cfg()


def _build(C, flags, k, lidar=False, seed=41):
    """tests/test_uncertainty._build_uc_net for k classes (the caller's cfg_reset restores cfg)."""
    from faster_rcnn_pytorch_multimodal_amd.utils.init_utils import seeded_state_dict
    C.cfg.NET_TYPE = "lidar" if lidar else "image"
    for name, v in flags.items():
        C.cfg.UC[name] = v
    if lidar:
        from faster_rcnn_pytorch_multimodal_amd.nets.lidarnet import lidarnet
        net = lidarnet(num_layers=101)
        net.create_architecture(k, tag="default", anchor_scales=C.cfg.LIDAR.ANCHOR_SCALES[0],
                                anchor_ratios=C.cfg.LIDAR.ANCHOR_ANGLES)
    else:
        from faster_rcnn_pytorch_multimodal_amd.nets.imagenet import imagenet
        net = imagenet(num_layers=101)
        net.create_architecture(k, tag="default", anchor_scales=C.cfg.ANCHOR_SCALES, anchor_ratios=C.cfg.ANCHOR_RATIOS)
    sd = seeded_state_dict(net, seed, bn_mode="tame")
    g = torch.Generator().manual_seed(seed)
    for name in sd:                       # non-degenerate heads (their reference init is N(0, 0.01))
        if any(t in name for t in ("_fc1", "_fc2", "al_var_net", "cls_score_net", "bbox_pred_net")) and name.endswith("weight"):
            sd[name] = torch.randn(sd[name].shape, generator=g) * (0.02 if "fc" in name else 0.004)
        if any(t in name for t in ("bbox_bn", "cls_bn")):
            if name.endswith("running_var"):
                sd[name] = torch.rand(sd[name].shape, generator=g) + 0.5
            elif name.endswith("running_mean") or name.endswith("bias"):
                sd[name] = torch.randn(sd[name].shape, generator=g) * 0.1
            elif name.endswith("weight"):
                sd[name] = torch.rand(sd[name].shape, generator=g) + 0.5
    net.load_state_dict(sd, strict=True)
    net.eval()
    net._device = DEV
    net.to(DEV)
    return net, sd


def _image_blobs(seed=8, classes=(3, 17)):
    rng = np.random.default_rng(seed)
    data = (rng.standard_normal((1, IMG_H, IMG_W, 3)) * 50).astype(np.float32)
    gt = np.array([[20, 30, 120, 110, classes[0]], [100, 40, 200, 150, classes[1]]], np.float32)
    return {"data": data, "info": IMG_INFO, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}


def _lidar_blobs(classes):
    import test_gpu_parity as T
    data, info, gt, _, _, _ = T._lidar_train_case(None)
    gt = gt.copy()
    gt[:, 7] = np.asarray(classes, np.float32)[np.arange(len(gt)) % len(classes)]
    return {"data": data, "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}


def _count_calls(monkeypatch):
    from faster_rcnn_pytorch_multimodal_amd import ops
    calls = {"wide": 0, "narrow": 0}

    def counted(name, fn):
        def inner(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return inner
    monkeypatch.setattr(ops, "bayesian_cross_entropy_wide", counted("wide", ops.bayesian_cross_entropy_wide))
    monkeypatch.setattr(ops, "bayesian_cross_entropy", counted("narrow", ops.bayesian_cross_entropy))
    return calls


@pytest.mark.parametrize("name,flags,k,lidar,classes,wide", [
    ("image21-al", AL, 21, False, (3, 17), True), ("image21-all", ALL_FLAGS, 21, False, (3, 20), True),
    ("lidar17-cls", CLS_AL, 17, True, (5, 16), True), ("lidar9-cls", CLS_AL, 9, True, (2, 8), False)])
def test_train_step(hip, cfg_reset, monkeypatch, name, flags, k, lidar, classes, wide):
    """One eager training step: the kernel the class count asks for runs, the classification loss equals the oracle's
    Bayesian cross entropy on the step's own logits, log-variances and seed, and the gradients of cls_score_net and
    cls_al_var_net equal float64 autograd of that loss through O.UcHeadsOracle's heads on the step's own head input."""
    from faster_rcnn_pytorch_multimodal_amd.nets import uncertainty as U
    C = cfg_reset
    net, sd = _build(C, flags, k, lidar)
    C.cfg.TRAIN.USE_GT = True              # ground-truth boxes join the proposals: the batch has foreground RoIs
    calls = _count_calls(monkeypatch)
    seen = {}
    inner = U.multi_head_train

    def recording(x2d, net_, modules, cache_name):
        if net_.cls_score_net in modules:
            seen["x"] = x2d.detach().clone()
        return inner(x2d, net_, modules, cache_name)
    monkeypatch.setattr(U, "multi_head_train", recording)
    net.train()
    blobs = _lidar_blobs(classes) if lidar else _image_blobs(classes=classes)

    def forward():
        net.set_uc_seed(123)
        net.zero_grad()
        torch.manual_seed(7)
        net.forward(blobs["data"], blobs["info"], blobs["gt_boxes"], None, mode="TRAIN")
    forward()
    # The seeded heads see an untrained fc7 whose scale nobody chose: log-variances of 6 and more, where every sample's
    # softmax is one-hot and the float64 reference itself is ill-conditioned.  Put the two class heads into the regime the
    # kernel tests pin (tests/test_loss_stat_kernels.bayes_case: |score| <= 4, log-variance around -0.5 +- 0.7) on this
    # step's own head input, like tests/test_many_classes._centred_heads, and run the step again.
    x0 = seen["x"].cpu().double()
    with torch.no_grad():
        for head, spread, centre in (("cls_score_net", 1.5, 0.0), ("cls_al_var_net", 0.7, -0.5)):
            lin = getattr(net, head)
            w = lin.weight.detach().cpu().double()
            w = w * (spread / float(((x0 - x0.mean(0)) @ w.t()).std()))
            b = centre - w @ x0.mean(0)
            lin.weight.copy_(w.float().to(DEV))
            lin.bias.copy_(b.float().to(DEV))
            sd[head + ".weight"], sd[head + ".bias"] = lin.weight.detach().cpu().clone(), lin.bias.detach().cpu().clone()
    calls["wide"] = calls["narrow"] = 0
    forward()
    assert calls == {"wide": int(wide), "narrow": int(not wide)}
    p, pt = net._predictions, net._proposal_targets
    labels = pt["labels"].cpu()
    assert int((labels > 0).sum()) > 0 and set(int(v) for v in labels.unique()) <= {0} | set(classes)
    s = int(C.cfg.UC.A_NUM_CE_SAMPLE)
    cs = p["cls_score"].detach().cpu().double()
    cv = p["cls_var"].detach().cpu().double()
    assert cs.shape[1] == k
    ce_ref, _ = O.bayesian_cross_entropy(cs, torch.exp(cv), labels, s, p["uc_seed"])
    ce = float(net._losses["cross_entropy"])
    print("%s: cross entropy %.6f, oracle %.6f" % (name, ce, float(ce_ref)))
    assert np.isfinite(ce) and abs(ce - float(ce_ref)) < 5e-5
    net.backward(net._losses["total_loss"])
    torch.cuda.synchronize()
    # float64 autograd through the oracle's two class heads on the device's own head input
    h = O.UcHeadsOracle(flags, num_classes=k, bbox_elem=7 if lidar else 4, lidar=lidar)
    own = h.state_dict()
    h.load_state_dict({n: sd[n] for n in own}, strict=True)
    h = h.double()
    x = seen["x"].cpu().double()
    cs64, cv64 = h.cls_score_net(x), h.cls_al_var_net(x)
    cs64.retain_grad(); cv64.retain_grad()
    loss64, _ = O.bayesian_cross_entropy(cs64, torch.exp(cv64), labels, s, p["uc_seed"])
    loss64.backward()
    assert abs(float(loss64) - float(ce_ref)) < 5e-5
    print("%s: |cls_score| <= %.2f, log-variance in [%.2f, %.2f]" % (name, float(cs.abs().max()), float(cv.min()), float(cv.max())))
    assert float(cs.abs().max()) <= 10.0 and float(cv.max()) <= 4.0
    # the kernel on the step's own inputs: per-element gradients at the Bayesian cross entropy's bars, 2e-6 * max(1, max |ref|)
    from faster_rcnn_pytorch_multimodal_amd import ops
    run = ops.bayesian_cross_entropy_wide if wide else ops.bayesian_cross_entropy
    _, dcs, dcv = run(p["cls_score"].detach().contiguous(), p["cls_var"].detach().contiguous(), pt["labels"], s, p["uc_seed"],
                      U.STREAM["bayes_ce"], var_is_log=True)
    elem_bar = {}
    for what, got, ref in (("cls_score_net", dcs, cs64.grad), ("cls_al_var_net", dcv, cv64.grad)):
        elem_bar[what] = 2e-6 * max(1.0, float(ref.abs().max()))
        err = float((got.cpu().double() - ref).abs().max())
        print("%s: d loss / d %s output: max |ref| %.3e, error %.3e (bar %.3e)" % (name, what, float(ref.abs().max()), err,
                                                                                   elem_bar[what]))
        assert err <= elem_bar[what], (what, err)
    # the parameter gradients are X^T d: an error of d within its bar reaches them multiplied by sum_n |x[n, c]| (1 for the
    # bias: sum over n of 1 per row, i.e. N), beside the fp32 GEMM's own rounding, 2e-5 * max(1, max |ref|)
    col_sum = float(x.abs().sum(0).max())
    for head in ("cls_score_net", "cls_al_var_net"):
        for part, gain in (("weight", col_sum), ("bias", float(x.shape[0]))):
            got = getattr(getattr(net, head), part).grad.cpu().double()
            ref = getattr(getattr(h, head), part).grad
            bar = elem_bar[head] * gain + 2e-5 * max(1.0, float(ref.abs().max()))
            err = float((got - ref).abs().max())
            print("%s: d %s.%s max |ref| %.3e, error %.3e (bar %.3e)" % (name, head, part, float(ref.abs().max()), err, bar))
            assert float(ref.abs().max()) > 0 and err <= bar, (head, part, err, bar)
    for head in ("bbox_pred_net",) + (("bbox_al_var_net",) if flags.get("EN_BBOX_ALEATORIC") else ()):
        gparam = getattr(net, head).weight.grad
        assert gparam is not None and bool(torch.isfinite(gparam).all()) and float(gparam.abs().max()) > 0, head


def _head_grads(net):
    return {n: getattr(net, n).weight.grad.detach().clone() for n in ("cls_score_net", "cls_al_var_net", "bbox_pred_net",
                                                                      "bbox_al_var_net")}


def test_captured_21_class_step_equals_the_eager_step_and_redraws(hip, cfg_reset, monkeypatch):
    """``enable_train_graphs()`` on the 21-class aleatoric detector: no eager fallback; the replayed step's four losses and the
    gradients of the four heads equal the eager step of the same seed bit for bit (the layers below the RoI pooling
    accumulate with float atomics: their gradients follow at tests/test_train_graphs.py's 1e-4); a replay with another seed
    draws other eps; the same step runs in TrainPipeline.  cfg.TRAIN.USE_GT stays off here: a captured step
    appends its capacity-padded gt buffer to the proposals, so the sampled RoIs sit in other rows than in the eager step and
    draw other eps (the draw index contains the row), whatever the class count."""
    from faster_rcnn_pytorch_multimodal_amd.model.train_graph import TrainPipeline
    from test_train_graphs import _grad_dev
    C = cfg_reset
    net_g, sd = _build(C, AL, 21)
    net_e, _ = _build(C, AL, 21)
    calls = _count_calls(monkeypatch)
    for n in (net_e, net_g):
        n.train()
    net_g.enable_train_graphs(True)
    opts = [torch.optim.SGD([p for p in n.parameters() if p.requires_grad], lr=1e-3) for n in (net_e, net_g)]
    blobs = _image_blobs()
    ce = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")                  # an eager fallback would warn
        for it, seed in enumerate((123, 123, 99991)):
            for o in opts:
                o.zero_grad(set_to_none=False)
            losses, terms = [None, None], [None, None]
            for idx in (1, 0):                          # graph net first: its warm-up tunes the plans both then use
                net = (net_e, net_g)[idx]
                torch.manual_seed(500)
                net.set_uc_seed(seed)
                losses[idx] = net.train_step(blobs, opts[idx], update_weights=False)
                terms[idx] = {n: v.detach().clone() for n, v in net._losses.items()}
            torch.cuda.synchronize()
            assert np.isfinite(losses[0])
            for n in terms[0]:
                assert torch.equal(terms[0][n].reshape(-1), terms[1][n].reshape(-1)), (it, n, terms[0][n], terms[1][n])
            ge, gg = _head_grads(net_e), _head_grads(net_g)
            for n in ge:
                assert torch.equal(ge[n], gg[n]), (it, n, float((ge[n] - gg[n]).abs().max()))
            worst, wname = _grad_dev(net_e, net_g)
            print("captured against eager step %d: loss %.6f, worst gradient deviation %.3g (%s)" % (it, losses[0], worst, wname))
            assert worst <= 1e-4, (it, wname, worst)
            ce.append(float(terms[1]["cross_entropy"]))
    assert len(net_g._train_graphs) == 1 and calls["narrow"] == 0 and calls["wide"] >= 4
    assert ce[0] == ce[1] and ce[2] != ce[0]            # the same seed replays the same eps, another seed draws others
    # the pipeline: two frames in flight, each the eager step's loss
    net_p, _ = _build(C, AL, 21)
    net_p.train()
    for prm in net_p.parameters():
        if prm.requires_grad:
            prm.grad = torch.zeros_like(prm)
    pipe = TrainPipeline(net_p, slots=2)
    torch.manual_seed(500)
    net_p.set_uc_seed(123)
    for _ in range(2):
        pipe.submit(blobs)
    got = [pipe.collect()[0] for _ in range(2)]
    pipe.flush()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in got)
    g = net_p.cls_al_var_net.weight.grad
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_21_class_test_frame_uncertainty_columns(hip, cfg_reset):
    """All four flags on a 21-class TEST frame: the uncertainty terms equal the oracle heads' on the device's own fc7, every
    detection's columns are its RoI's terms (its class's slice of the box variances) and so equal the oracle's, and the
    captured frame equals the eager frame bit for bit."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FramePool
    from faster_rcnn_pytorch_multimodal_amd.model.test import detect_frame_device
    from faster_rcnn_pytorch_multimodal_amd.nets import uncertainty as U
    C = cfg_reset
    k, e, thresh, max_dets = 21, 4, 0.02, 100
    net, sd = _build(C, ALL_FLAGS, k, seed=31)
    data = torch.from_numpy((np.random.default_rng(4).standard_normal((1, IMG_H, IMG_W, 3)) * 50).astype(np.float32)).to(DEV)
    t_mc = int(C.cfg.UC.E_NUM_SAMPLE)
    net.set_uc_seed(77)
    net.set_e_num_sample(t_mc)
    _, cls_prob, pred_boxes, rois, unc = net.test_frame(data, IMG_INFO)
    net.set_e_num_sample(1)
    n = rois.shape[0]
    assert list(unc.keys()) == list(U.UNCERTAINTY_ORDER) and unc["a_cls_var"].shape == (n, k) and unc["e_bbox_var"].shape == (n, k * e)
    h = O.UcHeadsOracle(ALL_FLAGS, num_classes=k, bbox_elem=e, lidar=False)
    h.load_state_dict({name: sd[name] for name in h.state_dict()}, strict=True)
    fc7 = net._predictions["fc7_uc"].cpu()
    _, cp_r, _, _, unc_r = h.test(fc7[:n], t_mc, C.cfg.UC.A_NUM_CE_SAMPLE, 77, O.BBOX_NORMALIZE_STDS, O.BBOX_NORMALIZE_MEANS)
    np.testing.assert_allclose(cls_prob.cpu().numpy(), cp_r.numpy(), rtol=0, atol=1e-5)
    tol = lambda v: 2e-5 * max(1.0, float(v.abs().max()))
    for name, v in unc_r.items():
        np.testing.assert_allclose(unc[name].cpu().numpy(), v.numpy(), rtol=1e-4, atol=tol(v), err_msg=name)
    # the eager frame with its filter; the RoI of every detection from the same filter run directly
    net.set_uc_seed(77)
    dets, counts = detect_frame_device(net, data, IMG_INFO, thresh, max_dets, max_dets)
    dets, counts = dets.clone(), counts.clone()
    p = net._predictions
    n_uc = U.num_uncertainty_pos(k, e)
    assert dets.shape == (k, max_dets, 5 + n_uc) and n_uc == 2 * (2 + k) + 2 * e
    assert int(counts[1:].sum()) > 0 and int((counts[1:] > 0).sum()) >= 2            # detections of several classes
    bare, bare_counts, det_roi = ops.filter_per_class(p["pred_boxes"].clone(), p["cls_prob"], float(IMG_W), float(IMG_H), 1.0,
                                                      thresh, C.cfg.TEST.NMS_THRESH, max_dets, max_dets,
                                                      roi_count=p["rois_count"], want_rois=True)
    assert torch.equal(bare_counts, counts) and torch.equal(bare, dets[..., :5])
    unc_d = p["uncertainties"]
    checked = 0
    for j in range(1, k):
        c = int(counts[j])
        assert bool((det_roi[j, :c] >= 0).all()) and bool((det_roi[j, c:] == -1).all())
        assert bool((dets[j, c:, 5:].contiguous().view(torch.int32) == 0).all())      # padding: +0.0
        roi = det_roi[j, :c].long()
        col = 5
        for name in U.UNCERTAINTY_ORDER:
            v, v_r = unc_d[name], unc_r[name]
            if name.endswith("bbox_var"):
                v, v_r = v[:, j * e:(j + 1) * e], v_r[:, j * e:(j + 1) * e]
            elif v.dim() == 1:
                v, v_r = v.unsqueeze(1), v_r.unsqueeze(1)
            w = v.shape[1]
            got = dets[j, :c, col:col + w]
            assert torch.equal(got, v[roi]), (j, name)                                # a copy of the frame's own terms
            if c:
                np.testing.assert_allclose(got.cpu().numpy(), v_r[roi.cpu()].numpy(), rtol=1e-4, atol=tol(unc_r[name]),
                                           err_msg="%s class %d" % (name, j))
            col += w
        assert col == 5 + n_uc
        checked += c
    assert checked == int(counts[1:].sum())
    # captured: the frame's draws come through the device word, the columns through one launch
    net.set_e_num_sample(t_mc)                           # lib/model/test.py:74-77, as test_net sets it around its frames
    try:
        pool = FramePool(net, streams=1, capture_after=1, autotune=False)
        runner = pool.runner((1, IMG_H, IMG_W, 3), IMG_INFO, thresh, max_dets)
        assert runner is not None and runner.graph is not None and not pool.uncapturable
        for _ in range(2):
            net.set_uc_seed(77)
            g_d, g_c = runner.run(data, poison=True)
            torch.cuda.synchronize()
            assert torch.equal(g_c, counts) and torch.equal(g_d.view(torch.int32), dets.view(torch.int32))
    finally:
        net.set_e_num_sample(1)
