"""Captured training steps beyond one frozen-BatchNorm image problem.

  * one graph per frame geometry serves every number of ground-truth boxes (padded gt buffer + device-side count);
  * the LiDAR detector's step (BatchNorm on batch statistics, 3-D targets) and FIXED_BLOCKS = -1 are capturable;
  * the uncertainty heads' draws reach a captured step through a device word;
  * a single-chain capture that contains runtime memset nodes is refused (the root cause of round 3's replay fault).
"""
import warnings

import numpy as np
import pytest
import torch

import test_gpu_parity as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _grad_dev(net_a, net_b):
    floor = 0.01 * max([float(p.grad.abs().max()) for p in net_a.parameters() if p.requires_grad and p.grad is not None] + [1e-30])
    worst, name_w = 0.0, None
    for (name, pa), (_, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
        if pa.requires_grad and pa.grad is not None:
            assert pb.grad is not None, name
            d = float((pa.grad - pb.grad).abs().max()) / max(float(pa.grad.abs().max()), floor)
            if d > worst:
                worst, name_w = d, name
    return worst, name_w


def test_one_captured_step_serves_every_gt_count(hip):
    """lib/roi_data_layer/minibatch.py:210-214: the number of gt boxes varies per frame.  Frames with 4, 1, 9 and 30 boxes
    replay ONE graph (gt buffer of 32 rows + device-side count) and give the eager step's losses and gradients; a frame
    with 40 boxes gets a second graph (capacity 64)."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    net_e, _ = T._build_fpn_pair(seed=23)
    net_g, _ = T._build_fpn_pair(seed=23)
    data, info, gt4, _, _ = T._fpn_case()
    rng = np.random.default_rng(3)

    def boxes(n):
        wh = rng.uniform(20, 120, (n, 2))
        xy = rng.uniform(0, 1, (n, 2)) * (np.array([320, 256]) - wh - 1)
        return np.concatenate((xy, xy + wh, np.ones((n, 1))), 1).astype(np.float32)

    gts = [gt4, boxes(1), boxes(9), boxes(30), boxes(40)]
    for n in (net_e, net_g):
        n.train()
    net_g.enable_train_graphs(True)
    opts = [torch.optim.SGD([p for p in n.parameters() if p.requires_grad], lr=1e-3) for n in (net_e, net_g)]
    for it, gt in enumerate(gts):
        blobs = {"data": data * (1.0 + 0.1 * it), "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
        for o in opts:
            o.zero_grad(set_to_none=False)
        losses = [None, None]
        for idx in (1, 0):                              # graph net first: its warm-up tunes the plans both then use
            torch.manual_seed(200 + it)
            losses[idx] = (net_e, net_g)[idx].train_step(blobs, opts[idx], update_weights=False)
        assert abs(losses[0] - losses[1]) <= 2e-5 * max(1.0, abs(losses[0])), (it, losses)
        worst, name = _grad_dev(net_e, net_g)
        assert worst <= 1e-4, (it, len(gt), name, worst)
    keys = sorted(k[3] for k in net_g._train_graphs)
    assert keys == [32, 64], keys
    # every runner counted its filter-gradient tiles in counters of its own, and every launch left them zero again
    torch.cuda.synchronize()
    assert all(r.inline and r.edges == r.nodes - 1 for r in net_g._train_graphs.values())     # train_step's graphs are ONE chain
    arenas = [r.wgrad_counters for r in net_g._train_graphs.values()]
    assert len({a.ints.data_ptr() for a in arenas}) == 2
    for a in arenas:
        assert a.cursor > 0 and int(a.ints.abs().max()) == 0
    C.reset_cfg()


def test_lidar_train_step_as_hipgraph_equals_eager_step(hip):
    """The LiDAR detector's step (lib/nets/lidarnet.py:153-181: layer2/3 BatchNorm on batch statistics; 3-D regression
    targets, proposal_target_layer.py:142-154) as a replayed graph: losses, gradients (incl. the BatchNorm affine
    parameters) and the running statistics follow the eager step over three frames with different numbers of boxes."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import train_graph
    net_e, oracle = T._build_lidar_pair(seed=9)
    net_g, _ = T._build_lidar_pair(seed=9)
    data, info, gt, _, _, _ = T._lidar_train_case(oracle)
    for n in (net_e, net_g):
        n.train()
    assert any(m.training for m in net_g.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert train_graph.graphable(net_g, {"gt_boxes": gt}) is None
    net_g.enable_train_graphs(True)
    opts = [torch.optim.SGD([p for p in n.parameters() if p.requires_grad], lr=1e-4) for n in (net_e, net_g)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                  # an eager fallback would warn
        for it, g in enumerate((gt, gt[:2], gt[1:4])):
            blobs = {"data": data * (1.0 + 0.2 * it), "info": info, "gt_boxes": g, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
            for o in opts:
                o.zero_grad(set_to_none=False)
            losses = [None, None]
            for idx in (1, 0):
                torch.manual_seed(300 + it)
                losses[idx] = (net_e, net_g)[idx].train_step(blobs, opts[idx], update_weights=False)
            assert np.isfinite(losses[0]) and abs(losses[0] - losses[1]) <= 5e-5 * max(1.0, abs(losses[0])), (it, losses)
            worst, name = _grad_dev(net_e, net_g)
            assert worst <= 2e-3, (it, name, worst)     # batch statistics over 13 x 11 positions amplify rounding
            for (k, be), (_, bg) in zip(net_e.named_buffers(), net_g.named_buffers()):
                if k.endswith("running_mean") or k.endswith("running_var"):
                    assert torch.allclose(be, bg, rtol=1e-4, atol=1e-5), (it, k)
                if k.endswith("num_batches_tracked"):
                    assert int(be) == int(bg) == it + 1 or int(be) == int(bg), k
    assert len(net_g._train_graphs) == 1
    # eval after the replays: the folded BatchNorm terms follow the statistics the graph updated
    net_e.eval(); net_g.eval()
    out_e = net_e.test_frame(data, info)
    out_g = net_g.test_frame(data, info)
    assert (out_e[1] - out_g[1]).abs().max().item() <= 1e-4
    C.reset_cfg()


def test_train_step_with_all_batchnorms_trainable_as_hipgraph(hip):
    """cfg.RESNET.FIXED_BLOCKS = -1 (lib/nets/imagenet.py:96-116,138-163: the stem's BatchNorm and every block train on
    batch statistics; non-FPN detector with layer4 as the tail): the step is capturable and follows the eager step."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    net_e, _ = T._build_pair(seed=51, fixed_blocks=-1)
    net_g, _ = T._build_pair(seed=51, fixed_blocks=-1)
    data, info, gt, _, _ = T._fpn_case()
    for n in (net_e, net_g):
        n.train()
    assert net_g.resnet.bn1.training and net_g.resnet.layer3[5].bn2.training
    net_g.enable_train_graphs(True)
    opts = [torch.optim.SGD([p for p in n.parameters() if p.requires_grad], lr=1e-4) for n in (net_e, net_g)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for it in range(2):
            blobs = {"data": data * (1.0 + 0.3 * it), "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
            for o in opts:
                o.zero_grad(set_to_none=False)
            losses = [None, None]
            for idx in (1, 0):
                torch.manual_seed(400 + it)
                losses[idx] = (net_e, net_g)[idx].train_step(blobs, opts[idx], update_weights=False)
            assert np.isfinite(losses[0]) and abs(losses[0] - losses[1]) <= 5e-5 * max(1.0, abs(losses[0])), (it, losses)
            worst, name = _grad_dev(net_e, net_g)
            assert worst <= 2e-3, (it, name, worst)
            for (k, be), (_, bg) in zip(net_e.named_buffers(), net_g.named_buffers()):
                if k.endswith("running_mean") or k.endswith("running_var"):
                    assert torch.allclose(be, bg, rtol=1e-4, atol=1e-5), (it, k)
    assert len(net_g._train_graphs) == 1
    C.reset_cfg()


def test_single_chain_capture_with_memset_nodes_is_refused(hip):
    """frcnn_set_memops_mode(1) makes the library initialise device memory with hipMemsetAsync / hipMemcpyAsync again: the
    single-chain capture then holds memset nodes - the pattern that replays wrongly from the second replay on under the
    runtime's packet-captured path (tools/train_graph_trace.py --memops 1) - and TrainStepRunner(inline=True) refuses it;
    the forked capture (general replay path) of the same step stays available.  Default mode: kernel nodes only."""
    from faster_rcnn_pytorch_multimodal_amd import _hip
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model.train_graph import InlineCaptureUnsafe, TrainStepRunner, packet_capture_disabled
    lib = _hip.load()
    net, _ = T._build_fpn_pair(seed=23)
    net.train()
    data, info, gt, _, _ = T._fpn_case()
    assert lib.frcnn_get_memops_mode() == 0
    r = TrainStepRunner(net, 256, 320, 3, len(gt), info, inline=True)
    assert r.node_kinds.get("memset", 0) == 0 and r.edges == r.nodes - 1
    try:
        _hip.check(lib.frcnn_set_memops_mode(1), "frcnn_set_memops_mode")
        if packet_capture_disabled():
            pytest.skip("DEBUG_CLR_GRAPH_PACKET_CAPTURE=0: every graph takes the general replay path")
        with pytest.raises(InlineCaptureUnsafe):
            TrainStepRunner(net, 256, 320, 3, len(gt), info, inline=True, autotune=False)
        forked = TrainStepRunner(net, 256, 320, 3, len(gt), info, inline=False, autotune=False)
        assert forked.node_kinds.get("memset", 0) >= 3
    finally:
        _hip.check(lib.frcnn_set_memops_mode(0), "frcnn_set_memops_mode")
    C.reset_cfg()


def test_solver_validation_replays_captured_frames(hip, tmp_path):
    """SolverWrapper with validation frames (lib/model/train_val.py:402-445): ``run_eval`` goes through the captured forward
    pass of the frame pool, which follows the weight updates in between (refreshes > 0, no re-capture), and after training
    the replayed forward equals the eager one at the final weights."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import train_val
    net, _ = T._build_fpn_pair(seed=23)
    data, info, gt, _, _ = T._fpn_case()
    C.cfg.TRAIN.SNAPSHOT_ITERS = 1000
    C.cfg.TRAIN.LEARNING_RATE = 1e-4

    class Frames:
        def next(self):
            return {"data": data, "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}

    solver = train_val.SolverWrapper(net, 2, Frames(), val_frames=Frames(), output_dir=str(tmp_path), batch_size=2, sum_size=0,
                                     val_sum_size=2, val_batch_size=2, log=lambda *_: None)
    losses = solver.train_model(5)
    assert len(losses) == 5 and all(np.isfinite(l) for l in losses)
    st = net.frame_pool().stats
    assert st["replays"] >= 4 and st["captures"] == 1 and st["refreshes"] >= 1 and st["invalidations"] == 0, st
    assert [v for it, k, v in solver.val_summaries if k == "val_num_rois"]
    blobs = Frames().next()
    out_g = net.run_eval(blobs, 1, update_summaries=False)
    net.enable_frame_graphs(False)
    out_e = net.run_eval(blobs, 1, update_summaries=False)
    assert torch.equal(out_g[1], out_e[1]) and torch.equal(out_g[3], out_e[3]) and torch.equal(out_g[4], out_e[4])
    assert net.training                                             # run_eval put the module back into train() mode
    C.reset_cfg()


def test_train_pipeline_updates_batchnorm_statistics_in_frame_order(hip):
    """BatchNorm on batch statistics (LiDAR layer2/3, lib/nets/lidarnet.py:152-175) with four captured steps in flight
    (cfg.TRAIN.FRAMES_IN_FLIGHT, the solver's default: one per hardware queue): the slots' replays overlap, so the running statistics must not be
    read-modify-written by the captured launches themselves (lost updates, lost counts).  Every slot leaves its frame's batch
    statistics in private buffers and the pipeline folds them in submission order - after 7 strongly different frames the
    running statistics and num_batches_tracked equal those of the sequential eager loop (the reference's per-frame update)."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model.train_graph import TrainPipeline
    net_e, oracle = T._build_lidar_pair(seed=9)
    net_p, _ = T._build_lidar_pair(seed=9)
    data, info, gt, _, _, _ = T._lidar_train_case(oracle)
    for n in (net_e, net_p):
        n.train()
    frames = [{"data": data * (1.0 + 0.6 * it), "info": info, "gt_boxes": (gt, gt[:2], gt[1:4])[it % 3],
               "gt_boxes_dc": np.zeros((0, 4), np.float32)} for it in range(7)]
    assert C.cfg.TRAIN.FRAMES_IN_FLIGHT == 4
    pipe = TrainPipeline(net_p, slots=int(C.cfg.TRAIN.FRAMES_IN_FLIGHT))
    assert pipe.distinct_queues == 4                          # every slot's stream on a hardware queue of its own
    torch.manual_seed(91)
    for b in frames:
        if pipe.in_flight() >= pipe.slots:
            pipe.collect()
        pipe.submit(b)
    assert all(r.bn_private is not None for slot in pipe.runners for r in slot.values())
    while pipe.in_flight():
        loss, _ = pipe.collect()
        assert np.isfinite(loss)
    pipe.flush()
    torch.cuda.synchronize()
    opt = torch.optim.SGD([p for p in net_e.parameters() if p.requires_grad], lr=1e-4)
    opt.zero_grad(set_to_none=False)
    torch.manual_seed(91)                                     # the same sampling seeds, frame by frame
    for b in frames:
        net_e.train_step(b, opt, update_weights=False)
    torch.cuda.synchronize()
    checked = equal = 0
    for (k, be), (_, bp) in zip(net_e.named_buffers(), net_p.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(be) == int(bp), (k, int(be), int(bp))
            if int(be):
                assert int(be) == len(frames), (k, int(be))
        if k.endswith("running_mean") or k.endswith("running_var"):
            checked += 1
            equal += int(torch.equal(be, bp))
            assert torch.allclose(be, bp, rtol=1e-5, atol=1e-7), (k, float((be - bp).abs().max()))
    moved = sum(int(m.num_batches_tracked) > 0 for m in net_p.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert moved >= 20 and checked >= 2 * moved
    print("pipeline vs sequential BatchNorm statistics: %d tensors compared, %d bit-equal, %d layers on batch statistics"
          % (checked, equal, moved))
    # the gradients of the pseudo batch agree as well (sum over the slots vs sequential accumulation)
    worst, name = _grad_dev(net_e, net_p)
    assert worst <= 5e-3, (name, worst)
    C.reset_cfg()


def test_captured_step_with_dont_care_boxes(hip):
    """cfg.TRAIN.IGNORE_DC (lib/layer_utils/proposal_target_layer.py:180-187: RoIs whose best overlap with a don't-care box
    reaches DC_THRESH are dropped before sampling; lib/roi_data_layer/minibatch.py:168-176 hands a varying number of such
    boxes per frame): the captured step holds a fixed-capacity don't-care buffer padded with a box no RoI overlaps, so frames
    with 0, 3 and 9 don't-care boxes replay ONE graph and follow the eager step - no eager fallback, no warning."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    net_e, _ = T._build_fpn_pair(seed=23)
    net_g, _ = T._build_fpn_pair(seed=23)
    C.cfg.TRAIN.IGNORE_DC = True
    C.cfg.TRAIN.DC_THRESH = 0.05                  # low bar + large boxes: an untrained RPN's proposals really get masked
    try:
        data, info, gt, _, _ = T._fpn_case()
        rng = np.random.default_rng(8)

        def dc_boxes(n):
            wh = rng.uniform(120, 250, (n, 2))
            xy = rng.uniform(0, 1, (n, 2)) * (np.array([320, 256]) - wh - 1)
            return np.concatenate((xy, xy + wh), 1).astype(np.float32)

        for n in (net_e, net_g):
            n.train()
        net_g.enable_train_graphs(True)
        opts = [torch.optim.SGD([p for p in n.parameters() if p.requires_grad], lr=1e-3) for n in (net_e, net_g)]
        masked = []
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            for it, n_dc in enumerate((3, 0, 9)):
                blobs = {"data": data * (1.0 + 0.1 * it), "info": info, "gt_boxes": gt, "gt_boxes_dc": dc_boxes(n_dc)}
                for o in opts:
                    o.zero_grad(set_to_none=False)
                losses = [None, None]
                for idx in (1, 0):
                    torch.manual_seed(500 + it)
                    losses[idx] = (net_e, net_g)[idx].train_step(blobs, opts[idx], update_weights=False)
                assert abs(losses[0] - losses[1]) <= 2e-5 * max(1.0, abs(losses[0])), (it, losses)
                worst, name = _grad_dev(net_e, net_g)
                assert worst <= 1e-4, (it, n_dc, name, worst)
                masked.append([int(v) for v in net_e._proposal_targets["counts"][:4].cpu()])
        assert len(net_g._train_graphs) == 1
        print("[sampled fg, sampled bg, fg candidates, bg candidates] with 3, 0, 9 don't-care boxes:", masked)
        cand = [m[2] + m[3] for m in masked]
        assert cand[1] > min(cand[0], cand[2])                          # the don't-care boxes really removed candidates
    finally:
        C.reset_cfg()


def test_chain_with_torch_memcpy_nodes_replays_bit_identically_on_four_streams(hip):
    """The captured steps still contain torch's own device-to-device ``copy_`` calls, i.e. hipGraph MEMCPY nodes (round 4's
    replay fault was traced to the library's memset / memcpy nodes inside single-chain graphs; the library now emits kernel
    nodes only, torch's copies remain).  Four single-chain graphs - library convolutions with torch ``copy_`` nodes between
    them - replayed 8 rounds on four streams with fresh inputs each round, no host synchronisation inside a round: every
    output equals the eager evaluation bit for bit, and the node census is what the test means to exercise."""
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import capture
    from faster_rcnn_pytorch_multimodal_amd.model.train_graph import graph_node_kinds
    ops = T._ops()
    g = torch.Generator().manual_seed(12)
    w1 = (torch.randn(256, 3, 3, 256, generator=g) / 48).to(DEV)
    w2 = (torch.randn(512, 1, 1, 256, generator=g) / 16).to(DEV)
    w3 = (torch.randn(256, 1, 1, 512, generator=g) / 22).to(DEV)
    sc, sh = (torch.rand(256, generator=g) + 0.5).to(DEV), torch.randn(256, generator=g).to(DEV)

    def chain(x, mid, mid2, out):
        y = ops.conv2d_nhwc(x, w1, sc, sh, None, stride=1, pad=1, relu=True)
        mid.copy_(y)                                             # torch D2D copy: a memcpy node inside the capture
        u = ops.conv2d_nhwc(mid, w2, None, None, None, relu=True)
        mid2.copy_(u)
        v = ops.conv2d_nhwc(mid2, w3, sc, sh, y, relu=True)
        out.copy_(v)

    n_streams, rounds = 4, 8
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    xs = [torch.zeros(1, 38, 63, 256, device=DEV) for _ in range(n_streams)]
    mids = [torch.zeros(1, 38, 63, 256, device=DEV) for _ in range(n_streams)]
    mid2s = [torch.zeros(1, 38, 63, 512, device=DEV) for _ in range(n_streams)]
    outs = [torch.zeros(1, 38, 63, 256, device=DEV) for _ in range(n_streams)]
    for k in range(n_streams):
        chain(xs[k], mids[k], mid2s[k], outs[k])                 # warm-up: plans, allocator
    torch.cuda.synchronize()
    graphs = []
    for k, st in enumerate(streams):
        st.wait_stream(torch.cuda.current_stream())
        gr = torch.cuda.CUDAGraph(keep_graph=True)
        with capture(gr, stream=st):
            chain(xs[k], mids[k], mid2s[k], outs[k])
        kinds, nodes, edges = graph_node_kinds(gr)
        assert kinds.get("memcpy", 0) >= 3 and kinds.get("memset", 0) == 0 and kinds.get("kernel", 0) >= 3, kinds
        assert edges == nodes - 1                                 # one chain
        gr.instantiate()
        graphs.append(gr)
    inputs = [[torch.randn(1, 38, 63, 256, generator=g).to(DEV) for _ in range(n_streams)] for _ in range(rounds)]
    torch.cuda.synchronize()
    got = []
    for r in range(rounds):
        for k, st in enumerate(streams):
            with torch.cuda.stream(st):
                xs[k].copy_(inputs[r][k], non_blocking=True)
                graphs[k].replay()
                got.append(outs[k].clone())
    torch.cuda.synchronize()
    ref_x, ref_mid, ref_mid2, ref_out = (torch.zeros_like(t) for t in (xs[0], mids[0], mid2s[0], outs[0]))
    for r in range(rounds):
        for k in range(n_streams):
            ref_x.copy_(inputs[r][k])
            chain(ref_x, ref_mid, ref_mid2, ref_out)
            torch.cuda.synchronize()
            assert torch.equal(got[r * n_streams + k], ref_out), (r, k)
    assert len({t.cpu().numpy().tobytes() for t in got}) == rounds * n_streams


def test_capture_collects_dead_graphs_first_and_holds_the_collector_off(hip):
    """model/frame_graph.capture: a dead reference cycle that owns a captured graph (what a dropped net and its cached
    TrainStepRunner are) must not be collected DURING a later capture - ``~CUDAGraph`` inside a global-mode capture is
    hipErrorStreamCaptureUnsupported and fatal, and torch >= 2.9 no longer collects before ``capture_begin``.  The helper
    collects it before the capture starts, keeps the cyclic collector off while capturing (autograd's backward thread
    allocates plenty of Python objects) and restores the collector's state afterwards, also when the body raises."""
    import gc
    import weakref
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import capture

    class Holder:
        pass

    x = torch.ones(1024, device=DEV)
    was = gc.isenabled()
    gc.disable()                                                  # so that the cycle below is still uncollected at capture()
    try:
        a, b = Holder(), Holder()
        a.other, b.other = b, a
        a.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(a.graph):
            a.y = x * 2
        dead = weakref.ref(a)
        del a, b
        assert dead() is not None                                 # garbage, but only the cyclic collector can free it
        gc.enable()
        seen = {}
        g2 = torch.cuda.CUDAGraph()
        with capture(g2):
            seen["alive"] = dead() is not None
            seen["collector"] = gc.isenabled()
            z = x + 1
        assert seen == {"alive": False, "collector": False}
        assert gc.isenabled()
        g2.replay()
        torch.cuda.synchronize()
        assert float(z[0]) == 2.0
        with pytest.raises(RuntimeError, match="stop"):
            with capture(torch.cuda.CUDAGraph()):
                _ = x + 2
                raise RuntimeError("stop")
        assert gc.isenabled()
        gc.disable()
        with capture(torch.cuda.CUDAGraph()):
            _ = x + 3
        assert not gc.isenabled()                                 # a caller that runs with the collector off stays that way
    finally:
        gc.enable() if was else gc.disable()


def test_filter_gradients_on_two_side_streams_equal_the_eager_step(hip):
    """autograd_ops.WGRAD_SIDE_STREAMS = 2: every parameter is pinned to one of two side streams, so launches into the same
    gradient buffer (the RPN head on five pyramid levels) stay ordered while different layers' filter gradients may overlap;
    their tile counters come from the runner's arena, one range per launch.  Losses and gradients of the replayed step follow
    the eager step over three frames."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import train_graph
    from faster_rcnn_pytorch_multimodal_amd.nets import autograd_ops
    net_e, _ = T._build_fpn_pair(seed=29)
    net_g, _ = T._build_fpn_pair(seed=29)
    data, info, gt, _, _ = T._fpn_case()
    for n in (net_e, net_g):
        n.train()
    net_g.enable_train_graphs(True)
    opts = [torch.optim.SGD([p for p in n.parameters() if p.requires_grad], lr=1e-3) for n in (net_e, net_g)]
    prev, supported = autograd_ops.WGRAD_SIDE_STREAMS, train_graph.inline_graphs_supported
    autograd_ops.WGRAD_SIDE_STREAMS = 2
    train_graph.inline_graphs_supported = lambda: False           # the FORKED capture (train_step's default is the single chain)
    try:
        for it in range(3):
            blobs = {"data": data * (1.0 + 0.1 * it), "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
            for o in opts:
                o.zero_grad(set_to_none=False)
            losses = [None, None]
            for idx in (1, 0):
                torch.manual_seed(400 + it)
                losses[idx] = (net_e, net_g)[idx].train_step(blobs, opts[idx], update_weights=False)
            assert abs(losses[0] - losses[1]) <= 2e-5 * max(1.0, abs(losses[0])), (it, losses)
            worst, name = _grad_dev(net_e, net_g)
            assert worst <= 1e-4, (it, name, worst)
        assert len(autograd_ops._SIDE[str(torch.device(DEV))]) == 2
        assert all(not r.inline for r in net_g._train_graphs.values())
    finally:
        autograd_ops.WGRAD_SIDE_STREAMS = prev
        train_graph.inline_graphs_supported = supported
        C.reset_cfg()


def test_concurrent_streams_are_chosen_by_measurement(hip):
    """model/streams.concurrent_streams: HIP streams share GPU_MAX_HW_QUEUES (4) hardware queues, and two streams on one
    queue run one after the other.  Of the streams torch hands out, some pairs are serialised (the probe must see that, or
    the premise is gone); the three / four streams picked for the pipelines overlap pairwise, measured again here with a
    longer kernel."""
    from faster_rcnn_pytorch_multimodal_amd.model import streams as S
    pool = [torch.cuda.Stream() for _ in range(10)]
    ser = S.serialised_pairs(pool)
    assert any(ser.values()) and not all(ser.values()), ser       # ten streams on four queues: some share, some do not
    for n in (3, 4):
        chosen, distinct = S.concurrent_streams(n, DEV)
        assert len(chosen) == n and len({s.cuda_stream for s in chosen}) == n
        assert distinct == n, (n, distinct)
        again = S.serialised_pairs(chosen, cycles=4 * S.PROBE_CYCLES)
        assert not any(again.values()), again
    seven, distinct = S.concurrent_streams(7, DEV)                 # more streams than queues: as many distinct as there are
    assert len(seven) == 7 and 3 <= distinct <= 7


def _replay_check_raising(monkeypatch, train_graph, error):
    def check(net, runner, blobs, grads):
        raise error

    monkeypatch.setattr(train_graph, "check_replays", check)


def test_replay_mismatch_falls_back_to_the_forked_capture(hip, monkeypatch):
    """train_graph.capture_with_fallback: a single-chain capture whose replay check reports ``ReplayMismatch`` (substituted
    here: the check raises on the host) is replaced, with ONE warning, by the forked capture - behind ``Network.train_step``
    (``captured_step``: the forked runner's loss follows the eager step's) and in ``TrainPipeline`` (the whole pipeline
    switches to forked graphs)."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import train_graph
    _replay_check_raising(monkeypatch, train_graph, train_graph.ReplayMismatch("replays differ (substituted check)"))
    net_e, _ = T._build_fpn_pair(seed=23)
    net_g, _ = T._build_fpn_pair(seed=23)
    data, info, gt, _, _ = T._fpn_case()
    for n in (net_e, net_g):
        n.train()
    blobs = {"data": data, "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        runner = train_graph.captured_step(net_g, 256, 320, 3, len(gt), info, blobs)
    assert len(seen) == 1 and "replays differ (substituted check)" in str(seen[0].message), [str(w.message) for w in seen]
    assert not runner.inline
    opt = torch.optim.SGD([p for p in net_e.parameters() if p.requires_grad], lr=1e-3)
    opt.zero_grad(set_to_none=False)
    torch.manual_seed(600)
    loss_e = net_e.train_step(blobs, opt, update_weights=False)
    torch.manual_seed(600)
    loss_g = float(runner.run(blobs)[0])
    assert abs(loss_e - loss_g) <= 2e-5 * max(1.0, abs(loss_e)), (loss_e, loss_g)
    pipe = train_graph.TrainPipeline(net_g, slots=1)
    assert pipe.inline
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        pipe.submit(blobs)
    loss_p, _ = pipe.collect()
    pipe.flush()
    assert len(seen) == 1 and np.isfinite(loss_p)
    assert not pipe.inline and [r.inline for r in pipe.runners[0].values()] == [False]
    C.reset_cfg()


def test_other_errors_of_the_replay_check_propagate_and_leave_no_trace(hip, monkeypatch):
    """Only ``InlineCaptureUnsafe`` and ``ReplayMismatch`` choose the forked capture: any other error of the check (here a
    substituted RuntimeError("boom")) reaches the caller of ``captured_step`` / ``TrainPipeline.submit`` - with every
    ``param.grad`` still the parameter's own buffer holding its bits, no deferred filter-gradient group and the eager
    schedule installed."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import train_graph
    from faster_rcnn_pytorch_multimodal_amd.nets import autograd_ops
    _replay_check_raising(monkeypatch, train_graph, RuntimeError("boom"))
    net, _ = T._build_fpn_pair(seed=23)
    net.train()
    data, info, gt, _, _ = T._fpn_case()
    blobs = {"data": data, "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
    params = [p for p in net.parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(5)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    own = [p.grad for p in params]
    before = [t.clone() for t in own]
    pipe = train_graph.TrainPipeline(net, slots=1)
    calls = (lambda: train_graph.captured_step(net, 256, 320, 3, len(gt), info, blobs), lambda: pipe.submit(blobs))
    for call in calls:
        with warnings.catch_warnings():
            warnings.simplefilter("error")                      # no fallback: nothing warns
            with pytest.raises(RuntimeError, match="^boom$") as raised:
                call()
        assert type(raised.value) is RuntimeError
        torch.cuda.synchronize()
        assert all(p.grad is o for p, o in zip(params, own))
        assert all(torch.equal(o, b) for o, b in zip(own, before))
        assert not autograd_ops._DEFER
        assert autograd_ops.SCHEDULE is autograd_ops.EAGER_SCHEDULE
    assert pipe.inline and not pipe.runners[0]                  # the pipeline did not switch, and kept no runner
    C.reset_cfg()
