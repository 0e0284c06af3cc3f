"""frcnn_conv2d_fwd_wres_pre / ops.conv2d_nhwc_winograd_res: the Winograd F(2x2,3x3) output transform with a residual operand
(csrc/conv_winograd.hip wino_output_kernel<true>) and the rule that sends a call there.

Shapes.  N in {1, 2} x (H, W) in {(1,1), (2,2), (3,3), (2,5), (5,4), (7,7)} x (C, K) in {(4,4), (8,36), (64,64)} - winograd_ok
admits all of them (C % 4 == 0, K % 4 == 0): a map smaller than a tile, one tile, odd x odd (interior, right, bottom and corner
tiles), odd in one direction only, a K that is no multiple of 32, and C % 32 == 0 for the fused input transform.  Every case
runs with trimming on and off, relu 0 / 1, and scale / shift present and NULL.

What is compared with what.
 * float operands (standard normal): the result is BIT-EQUAL to the existing residual-free call with relu = 0 followed by
   torch's float32 add and ReLU - one rounded add behind an unchanged v = o * scale + shift.
 * integer operands (the recipe of tests/test_conv_f32_exact.py: x, w, residual, shift in [-3, 3], scale in {0.5, 1, 2}; every
   Winograd intermediate is a multiple of 1/4 below 2^22): the result EQUALS float64, no tolerance.
 * forced implicit GEMM, and a cached implicit-GEMM plan under the residual-free key: bit-equal to ops.conv2d_nhwc(residual=).
 * cached Winograd plans: the fused input transform and the persistent tile against the un-fused 64x64 plan, bit-equal.
The output and the workspace lie between NaN guard bands, pre-filled with NaN; x, the residual and the filters are compared
with copies taken before the call.
"""
import ctypes
import itertools

import pytest

from guarded_buffers import DEV, guarded, guards_flag

BAND = 4096
BATCHES = (1, 2)
MAPS = ((1, 1), (2, 2), (3, 3), (2, 5), (5, 4), (7, 7))
CHANNELS = ((4, 4), (8, 36), (64, 64))
CASES = [(n, h, w, c, k) for n in BATCHES for (h, w) in MAPS for (c, k) in CHANNELS]
TRIMS = (0, 128)
SWITCHES = list(itertools.product((False, True), (False, True)))      # (relu, scale / shift present)
TWO22 = 1 << 22

_OPERANDS = {}


def case_id(case):
    return "n%d_%dx%d_c%d_k%d" % case


def lib():
    from faster_rcnn_pytorch_multimodal_amd import _hip
    return _hip.load()


def restore_hooks():
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    ops.set_conv_algo(0)
    ops.set_conv_autotune(False)
    _hip.check(lib().frcnn_conv2d_clear_plans(), "clear_plans")


@pytest.fixture
def hooks(hip):
    restore_hooks()
    try:
        yield
    finally:
        restore_hooks()


def operands(case):
    """Per case, made once and never modified: float operands, integer operands and the integer case's float64 results."""
    if case not in _OPERANDS:
        import torch
        import torch.nn.functional as F
        n, h, w, c, k = case
        gen = torch.Generator().manual_seed(7000 + CASES.index(case))
        ints = lambda *shape: torch.randint(-3, 4, shape, generator=gen).double()
        pow2 = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (k,), generator=gen)]
        randn = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float32)
        i = {"x": ints(n, h, w, c), "w": ints(k, 3, 3, c), "res": ints(n, h, w, k), "scale": pow2, "shift": ints(k)}
        assert 81 * 9 * c * 2 + 6 < TWO22                     # test_conv_f32_exact.exact_regime for a Winograd shape
        y = F.conv2d(i["x"].permute(0, 3, 1, 2), i["w"].permute(0, 3, 1, 2), stride=1, padding=1).permute(0, 2, 3, 1).contiguous()
        want = {}
        for relu, affine in SWITCHES:
            v = (y * i["scale"] + i["shift"] if affine else y) + i["res"]
            want[(relu, affine)] = (torch.relu(v) if relu else v).to(DEV)
        f = {"x": randn(n, h, w, c), "w": randn(k, 3, 3, c) * (2.0 / (9 * c)) ** 0.5, "res": randn(n, h, w, k),
             "scale": 0.5 + torch.rand((k,), generator=gen), "shift": randn(k)}
        to_dev = lambda d: {key: t.float().to(DEV).contiguous() for key, t in d.items()}
        _OPERANDS[case] = {"int": to_dev(i), "float": to_dev(f), "want64": want}
    return _OPERANDS[case]


def ws_floats_of(case):
    n, h, w, c, k = case
    nbytes = int(lib().frcnn_conv2d_fwd_ws_bytes(n, h, w, c, k, 3, 3, 1, 1, 0))      # after the hooks are set
    assert nbytes % 4 == 0
    return nbytes // 4


def run_wres(case, op, relu, affine, u=None):
    """The call under test inside guarded buffers.  Returns (flags tensor [bands of y, bands of ws, operands unchanged], y)."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k = case
    ws_floats = ws_floats_of(case)
    wbuf, ws = guarded(ws_floats, guard=BAND)
    obuf, out = guarded(n * h * w * k, guard=BAND)
    held = [op[key].clone() for key in ("x", "res", "w")] + ([u.clone()] if u is not None else [])
    got = ops.conv2d_nhwc_winograd_res(op["x"], op["w"], op["res"], op["scale"] if affine else None, op["shift"] if affine else None,
                                       relu=relu, out=out.view(n, h, w, k), w_winograd=u, ws=ws)
    assert got.data_ptr() == out.data_ptr()
    now = [op["x"], op["res"], op["w"]] + ([u] if u is not None else [])
    same = torch.stack([(a.view(torch.int32) == b.view(torch.int32)).all() for a, b in zip(held, now)]).all()
    flags = torch.stack([guards_flag(obuf, out.numel(), BAND), guards_flag(wbuf, ws_floats, BAND), same])
    return flags, got


def check_flags(label, flags):
    f = flags.tolist()
    assert f[0], "%s: wrote outside y" % label
    assert f[1], "%s: wrote outside the workspace" % label
    assert f[2], "%s: x, the residual or a filter changed" % label


def bits_equal(a, b):
    import torch
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def composed(op, relu, affine, **kw):
    """The existing residual-free call with relu = 0, then torch's float32 add and ReLU."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    base = ops.conv2d_nhwc(op["x"], op["w"], op["scale"] if affine else None, op["shift"] if affine else None, None, stride=1, pad=1,
                           relu=False, **kw)
    v = base + op["res"]
    return torch.relu(v) if relu else v


# ---- forced Winograd ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forced_winograd_is_the_residual_free_call_then_add_and_relu(hooks, case):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    ops_ = operands(case)
    u = {kind: ops.winograd_filter(ops_[kind]["w"]) for kind in ("int", "float")}
    for trim in TRIMS:
        ops.set_conv_algo(2 | trim)
        for relu, affine in SWITCHES:
            for filt in (False, True):
                label = "%s algo %d relu=%s affine=%s caller's filter=%s" % (case_id(case), 2 | trim, relu, affine, filt)
                flags, got = run_wres(case, ops_["float"], relu, affine, u["float"] if filt else None)
                want = composed(ops_["float"], relu, affine)
                check_flags(label, flags)
                assert not bool(torch.isnan(got).any()), label + ": an element of y was not written"
                assert bits_equal(got, want), label + ": differs from residual-free Winograd + float32 add + ReLU"
                flags, got = run_wres(case, ops_["int"], relu, affine, u["int"] if filt else None)
                check_flags(label + " (integers)", flags)
                assert bits_equal(got, composed(ops_["int"], relu, affine)), label + " (integers)"
                assert bool((got.double() == ops_["want64"][(relu, affine)]).all()), label + ": integers differ from float64"


# ---- the implicit GEMM where the residual-free call would not run Winograd ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_without_a_winograd_plan_it_is_the_residual_gemm(hooks, case):
    """Forced implicit GEMM (mode 1), no plan at all (mode 0, no autotuning: the analytic plan) and an imported implicit-GEMM
    plan under the residual-free key: bit-equal to ops.conv2d_nhwc(..., residual=...)."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k = case
    op = operands(case)["float"]
    key = [n, h, w, c, k, 3, 3, 1, 1]
    for setup in ("forced", "no plan", "gemm plan"):
        restore_hooks()
        if setup == "forced":
            ops.set_conv_algo(1)
        if setup == "gemm plan":
            ops.import_conv_plans([key + [1, 5, 1, (9 * c + 31) // 32]])
            assert ops.conv_plan_algo(n, h, w, c, k, 3, 3, 1, 1) == 0
        for relu, affine in SWITCHES:
            label = "%s %s relu=%s affine=%s" % (case_id(case), setup, relu, affine)
            flags, got = run_wres(case, op, relu, affine)
            want = ops.conv2d_nhwc(op["x"], op["w"], op["scale"] if affine else None, op["shift"] if affine else None, op["res"],
                                   stride=1, pad=1, relu=relu)
            check_flags(label, flags)
            assert bits_equal(got, want), label


# ---- cached Winograd plans ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cached_winograd_plans_fused_and_persistent_equal_the_unfused_one(hooks, case):
    """Plan rows under the RESIDUAL-FREE key (the residual key is not consulted): 64x64 un-fused (5 + 16), the persistent tile
    (13 + 16), and for C % 32 == 0 the fused input transform (5 + 32) - each equals residual-free + add + ReLU under the same
    plan, and the fused and persistent results equal the un-fused plan's bits."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k = case
    ops_ = operands(case)
    key = [n, h, w, c, k, 3, 3, 1, 1]
    codes = [5 + 16, 13 + 16] + ([5 + 32] if c % 32 == 0 else [])
    results = {}
    for code in codes:
        restore_hooks()
        # a residual-key GEMM row next to it: the call must not follow that one
        ops.import_conv_plans([key + [1, code, 1, (c + 31) // 32], key + [1 + 256, 5, 1, (9 * c + 31) // 32]])
        assert ops.conv_plan_algo(n, h, w, c, k, 3, 3, 1, 1) == 1 and ops.conv_plan_algo(n, h, w, c, k, 3, 3, 1, 1, True) == 0
        u = ops.winograd_filter(ops_["float"]["w"])
        for trim in TRIMS:
            ops.set_conv_algo(0 | trim)
            for relu, affine in SWITCHES:
                label = "%s plan code %d algo %d relu=%s affine=%s" % (case_id(case), code, trim, relu, affine)
                flags, got = run_wres(case, ops_["float"], relu, affine, u)
                check_flags(label, flags)
                assert not bool(torch.isnan(got).any()), label
                assert bits_equal(got, composed(ops_["float"], relu, affine, w_winograd=u)), label
                results[(code, trim, relu, affine)] = got.clone()
                flags, got = run_wres(case, ops_["int"], relu, affine)
                check_flags(label + " (integers)", flags)
                assert bool((got.double() == ops_["want64"][(relu, affine)]).all()), label + ": integers differ from float64"
    for (code, trim, relu, affine), got in results.items():
        assert bits_equal(got, results[(5 + 16, 0, relu, affine)]), (case_id(case), code, trim, relu, affine)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 2))
def test_a_new_shape_is_tuned_as_the_residual_free_call(hooks, mode):
    """Autotuning on, no plan yet: the call tunes its shape under the RESIDUAL-FREE key, as the residual-free call would (under
    forced Winograd the winner is a Winograd plan; with both forms allowed it is whichever is faster), and follows that plan:
    Winograd -> the residual-free call on the cached plan + add + ReLU, GEMM -> ops.conv2d_nhwc(residual=).  The result is
    complete whatever the tuner's candidates left in y."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    case = (2, 5, 4, 64, 64)
    n, h, w, c, k = case
    op = operands(case)["float"]
    ops.set_conv_algo(mode)
    ops.set_conv_autotune(True)
    assert ops.conv_plan_algo(n, h, w, c, k, 3, 3, 1, 1, False) == -1
    flags, got = run_wres(case, op, True, True)
    got = got.clone()
    ops.set_conv_autotune(False)
    check_flags("tuned, algo %d" % mode, flags)
    form = ops.conv_plan_algo(n, h, w, c, k, 3, 3, 1, 1, False)
    assert form == 1 if mode == 2 else form in (0, 1)
    if form == 1:
        assert ops.conv_plan_algo(n, h, w, c, k, 3, 3, 1, 1, True) == -1           # nothing was planned under the residual key
        want = composed(op, True, True)
    else:
        want = ops.conv2d_nhwc(op["x"], op["w"], op["scale"], op["shift"], op["res"], stride=1, pad=1, relu=True)
    assert not bool(torch.isnan(got).any()) and bits_equal(got, want)
    flags, again = run_wres(case, op, True, True)                                   # the cached plan, no tuning
    check_flags("cached, algo %d" % mode, flags)
    assert bits_equal(again, got)


# ---- non-finite residuals ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [(1, 1, 1, 4, 4), (2, 3, 3, 8, 36), (1, 7, 7, 64, 64), (2, 5, 4, 64, 64)], ids=case_id)
def test_nan_and_inf_in_the_residual_arrive_under_relu_f32s_rule(hooks, case):
    """NaN, +Inf and -Inf planted in res (the first, the middle and the last element, and one of each kind in between where
    the tensor has room): relu = 0 passes all three on; relu = 1 keeps NaN and +Inf and turns -Inf into 0 (relu(NaN) is NaN).
    Every other element keeps the bits it has with a finite residual."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k = case
    op = dict(operands(case)["float"])
    numel = n * h * w * k
    spots = {0: float("nan"), numel // 2: float("inf"), numel - 1: float("-inf")}
    if numel >= 8:
        spots.update({1: float("inf"), 2: float("-inf"), numel - 2: float("nan")})
    res = op["res"].clone()
    for at, v in spots.items():
        res.view(-1)[at] = v
    clean = op["res"]
    op["res"] = res
    for trim in TRIMS:
        ops.set_conv_algo(2 | trim)
        for relu, affine in SWITCHES:
            label = "%s algo %d relu=%s affine=%s" % (case_id(case), 2 | trim, relu, affine)
            flags, got = run_wres(case, op, relu, affine)
            check_flags(label, flags)
            flat = got.view(-1).cpu()
            for at, v in spots.items():
                if v != v:
                    assert flat[at] != flat[at], (label, at, float(flat[at]))
                elif v > 0:
                    assert float(flat[at]) == float("inf"), (label, at, float(flat[at]))
                else:
                    assert float(flat[at]) == (0.0 if relu else float("-inf")), (label, at, float(flat[at]))
            op_clean = dict(op, res=clean)
            want = composed(op_clean, relu, affine).view(-1).cpu()
            keep = torch.ones(numel, dtype=torch.bool)
            keep[list(spots)] = False
            assert bits_equal(flat[keep], want[keep]), label


# ---- stream capture ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [(2, 3, 3, 8, 36), (1, 7, 7, 64, 64)], ids=case_id)
def test_a_captured_call_replays_the_eager_bits_with_the_residual_free_calls_node_count(hooks, case):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.model.train_graph import graph_node_kinds
    n, h, w, c, k = case
    op = operands(case)["float"]
    ops.set_conv_algo(2)
    u = ops.winograd_filter(op["w"])
    eager = ops.conv2d_nhwc_winograd_res(op["x"], op["w"], op["res"], op["scale"], op["shift"], relu=True, w_winograd=u)
    ws = torch.empty(ws_floats_of(case) * 4, dtype=torch.uint8, device=DEV)
    out = {name: torch.empty((n, h, w, k), device=DEV) for name in ("wres", "free")}
    torch.cuda.synchronize()
    nodes = {}
    graphs = {}
    for name in ("wres", "free"):
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            if name == "wres":
                ops.conv2d_nhwc_winograd_res(op["x"], op["w"], op["res"], op["scale"], op["shift"], relu=True, out=out[name], w_winograd=u, ws=ws)
            else:
                ops.conv2d_nhwc(op["x"], op["w"], op["scale"], op["shift"], None, stride=1, pad=1, relu=True, out=out[name], w_winograd=u, ws=ws)
        kinds, count, _ = graph_node_kinds(graph)
        assert set(kinds) == {"kernel"}, kinds
        nodes[name] = count
        graph.instantiate()
        graphs[name] = graph
    assert nodes["wres"] == nodes["free"] >= 3, nodes            # input transform, grouped GEMM, output transform
    for _ in range(2):
        out["wres"].fill_(float("nan"))
        graphs["wres"].replay()
        torch.cuda.synchronize()
        assert bits_equal(out["wres"], eager)


# ---- rejections --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rejections_return_the_error_without_a_launch(hooks):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    n, h, w, c, k = 1, 3, 3, 8, 8
    x = torch.randn((n, h, w, c), device=DEV)
    res = torch.randn((n, h, w, k), device=DEV)
    obuf, y = guarded(n * h * w * k, guard=BAND)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(xp, wp, rp, yp, c_, k_, r_, s_, stride, pad):
        wt = torch.randn((max(k_, 1), r_, s_, max(c_, 1)), device=DEV)
        return lib().frcnn_conv2d_fwd_wres_pre(xp, wt.data_ptr() if wp else None, None, None, None, rp, yp, n, h, w, c_, k_, r_, s_,
                                               stride, pad, 0, 0, ws.data_ptr(), ws.numel(), stream)

    good = (x.data_ptr(), True, res.data_ptr(), y.data_ptr())
    for mode in (0, 1, 2):
        ops.set_conv_algo(mode)
        for label, args in (("null residual", (x.data_ptr(), True, None, y.data_ptr(), c, k, 3, 3, 1, 1)),
                            ("null filter", (x.data_ptr(), False, res.data_ptr(), y.data_ptr(), c, k, 3, 3, 1, 1)),
                            ("null x", (None, True, res.data_ptr(), y.data_ptr(), c, k, 3, 3, 1, 1)),
                            ("null y", (x.data_ptr(), True, res.data_ptr(), None, c, k, 3, 3, 1, 1)),
                            ("1x1", good + (c, k, 1, 1, 1, 0)),
                            ("3x1", good + (c, k, 3, 1, 1, 1)),
                            ("stride 2", good + (c, k, 3, 3, 2, 1)),
                            ("pad 0", good + (c, k, 3, 3, 1, 0)),
                            ("pad 2", good + (c, k, 3, 3, 1, 2)),
                            ("k % 4", good + (c, 6, 3, 3, 1, 1)),
                            ("c % 4", good + (6, k, 3, 3, 1, 1))):
            assert call(*args) == -1, (mode, label)                                   # FRCNN_ERR_ARG
            assert lib().frcnn_last_error(), label
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(guards_flag(obuf, y.numel(), BAND))     # nothing was launched into y
    ops.set_conv_algo(2)
    wt = torch.randn((k, 3, 3, c), device=DEV)
    for bad in (lambda: ops.conv2d_nhwc_winograd_res(x, wt, None),
                lambda: ops.conv2d_nhwc_winograd_res(x, wt, res[:, :2].contiguous()),
                lambda: ops.conv2d_nhwc_winograd_res(x, wt[:, :1].contiguous(), res),
                lambda: ops.conv2d_nhwc_winograd_res(x, wt, res, w_winograd=torch.zeros((16, k, c + 4), device=DEV)),
                lambda: ops.conv2d_nhwc_winograd_res(x.cpu(), wt, res)):
        with pytest.raises(_hip.HipError):
            bad()


@pytest.mark.gpu
def test_no_hook_is_left_set(hip):
    from faster_rcnn_pytorch_multimodal_amd import ops
    before = hip.frcnn_settings_signature()
    assert ops._CONV_ALGO_MODE == 0 and ops._CONV_ALGO_FLAGS == 0 and ops.export_conv_plans() == []
    ops.set_conv_algo(0)
    assert hip.frcnn_settings_signature() == before, "a convolution hook was left set"
