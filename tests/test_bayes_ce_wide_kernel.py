"""frcnn_bayesian_cross_entropy_wide (csrc/train_ops.hip: one wavefront per RoI, 2 <= K <= 1024) against the float64 reference
of tests/test_loss_stat_kernels.py (O.bayesian_cross_entropy + autograd on the replayed draws) at that file's bars
(loss 2e-5, dscore 2e-6, dvar 2e-6 / 5e-6, each times max(1, max |reference term|)), and bit for bit against the
one-thread-per-RoI kernel wherever both accept K.

Which case reaches which regime (N, K, S):
  (1,17,3) (3,17,7)      one class over the narrow limit; one / three live waves of a four-wave workgroup
  (5,21,200)             two workgroups, the second with one live wave; VOC's class count at A_NUM_CE_SAMPLE
  (7,64,20)              one class per lane exactly (no dead lane)
  (6,65,20)              a second slot with one live lane (template 2)
  (256,81,200)           the training batch at COCO's class count
  (9,128,5) (5,130,11)   template 2 full; template 4 with two live lanes in its third slot
  (4,1000,9) (2,1024,3)  template 16, partial and full
  narrow shapes          template 1 with K < 64: bit-equal to bayes_ce_kernel
The float32 CPU restatement meets every bar with 4x headroom (test_cpu_restatement_*), so a device miss is a finding about
the kernel and not about the bar.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import frcnn_oracle as O
from test_loss_stat_kernels import (BAYES_GRAD, BAYES_SEED, BAYES_SHAPES, BAYES_STREAM, HEADROOM, _bits_equal, _check_all,
                                    _scale, bayes_case, bayes_restate)

DEV = "cuda:0"
WIDE_SHAPES = [(1, 17, 3), (3, 17, 7), (5, 21, 200), (7, 64, 20), (6, 65, 20), (256, 81, 200), (9, 128, 5), (5, 130, 11),
               (4, 1000, 9), (2, 1024, 3)]
WIDE_CASES = [(s, m) for s in WIDE_SHAPES for m in ("logvar", "var")]
NARROW_SHAPES = list(BAYES_SHAPES) + [(3, 16, 1)]
assert NARROW_SHAPES[:3] == [(1, 2, 3), (257, 3, 50), (300, 16, 20)]
NARROW_CASES = [(s, m) for s in NARROW_SHAPES for m in ("logvar", "var")]
WIDE_LIMIT = 1024


def _id(c):
    return "N%d-K%d-S%d-%s" % (c[0] + (c[1],))


def _ops():
    from faster_rcnn_pytorch_multimodal_amd import ops
    return ops


def _hip_error():
    from faster_rcnn_pytorch_multimodal_amd import _hip
    return _hip.HipError


def _args(inp):
    return [inp[n].to(DEV) for n in ("score", "var", "labels")] + [inp["s"], BAYES_SEED, BAYES_STREAM]


def custom_case(score, logvar, labels, s, mode):
    """bayes_case's reference and bars for inputs given by the caller (planted labels, offset scores)."""
    n, k = score.shape
    sc = score.double().requires_grad_(True)
    if mode == "logvar":
        var_in = logvar
        leaf = logvar.double().requires_grad_(True)
        var64 = torch.exp(leaf)
    else:
        var_in = torch.exp(logvar)
        var_in.view(-1)[::5] = 0.0
        leaf = var_in.double().requires_grad_(True)
        var64 = leaf
    loss, _ = O.bayesian_cross_entropy(sc, var64, labels, s, BAYES_SEED, BAYES_STREAM)
    (BAYES_GRAD * loss).backward()
    with torch.no_grad():
        samples, _ = O.logit_distort_replay(score.double(), var64.detach(), s, BAYES_SEED, BAYES_STREAM)
        avg = F.softmax(samples, 2).mean(0).gather(1, labels.long().unsqueeze(1))
    assert float(avg.min()) > 1e-6
    dvar = leaf.grad.clone()
    zero_var = var_in == 0 if mode == "var" else torch.zeros_like(var_in, dtype=torch.bool)
    assert bool(torch.isfinite(dvar[~zero_var]).all())
    dvar[zero_var] = 0.0
    inp = dict(score=score, var=var_in.contiguous(), labels=labels, s=s, is_log=mode == "logvar", zero_var=zero_var)
    ref = dict(loss=loss.detach(), dscore=sc.grad, dvar=dvar)
    bars = dict(loss=2e-5 * _scale(-torch.log(avg)), dscore=2e-6 * _scale(sc.grad),
                dvar=(2e-6 if mode == "logvar" else 5e-6) * _scale(dvar))
    return inp, ref, bars


PLANTED = (0, 63, 64, 129)


@functools.lru_cache(maxsize=None)
def planted_case(mode):
    """K = 130: the target in the first and last lane of the first slot, the first lane of the second and the last class."""
    n, k, s = 6, 130, 11
    g = torch.Generator().manual_seed(130)
    score = torch.randn(n, k, generator=g).clamp(-4, 4)
    logvar = (torch.randn(n, k, generator=g) * 0.7 - 0.5).clamp(max=1.0)
    labels = torch.tensor([PLANTED[i % 4] for i in range(n)], dtype=torch.float32)
    return custom_case(score, logvar, labels, s, mode)


@functools.lru_cache(maxsize=None)
def offset_case(mode):
    """Scores that are multiples of 1/8 plus 128 on every class: expf(z) overflows without the maximum subtraction
    (exp(128) > FLT_MAX), and the float64 reference sees exactly the float32 inputs."""
    n, k, s = 9, 70, 20
    g = torch.Generator().manual_seed(128)
    score = torch.randint(-32, 33, (n, k), generator=g).float() / 8 + 128.0
    assert float(score.min()) >= 124 and torch.equal(score * 8, torch.round(score * 8))
    logvar = (torch.randn(n, k, generator=g) * 0.7 - 0.5).clamp(max=1.0)
    labels = torch.randint(0, k, (n,), generator=g).float()
    return custom_case(score, logvar, labels, s, mode)


# ---- without a GPU: the bars are reachable in float32 with 4x headroom -------------------------------------------------
@pytest.mark.parametrize("case", WIDE_CASES, ids=_id)
def test_cpu_restatement_wide_shapes(case):
    inp, ref, bars = bayes_case(*case)
    if case[1] == "var":
        assert int(inp["zero_var"].sum()) == (case[0][0] * case[0][1] + 4) // 5
    _check_all("bayes_wide", _id(case), bayes_restate(inp), ref, bars, "cpu32", HEADROOM)


@pytest.mark.parametrize("mode", ["logvar", "var"])
@pytest.mark.parametrize("builder", [planted_case, offset_case], ids=["planted", "offset"])
def test_cpu_restatement_planted_and_offset(builder, mode):
    inp, ref, bars = builder(mode)
    _check_all("bayes_wide", builder.__name__ + "-" + mode, bayes_restate(inp), ref, bars, "cpu32", HEADROOM)


def test_dispatch_rule_without_a_gpu():
    ops = _ops()
    assert [ops.bayes_ce_uses_wide_form(k) for k in (2, 9, 16, 17, 21, 81, 1024)] == [False] * 3 + [True] * 4
    assert ops.BAYES_CE_WIDE_MAX_CLASSES == WIDE_LIMIT


def test_argument_errors_are_reported_without_a_gpu():
    """Through the C ABI: every bad call returns FRCNN_ERR_ARG on the host, before any launch."""
    from faster_rcnn_pytorch_multimodal_amd import _hip
    lib = _hip.load()
    assert lib.frcnn_version() >= 124
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(5)]                  # never dereferenced
    good = dict(score=p[0], var=p[1], labels=p[2], n=4, k=17, s=3, loss=p[3], per_roi=p[4])

    def call(**kw):
        a = dict(good, **kw)
        return lib.frcnn_bayesian_cross_entropy_wide(a["score"], a["var"], a["labels"], a["n"], a["k"], a["s"], 1, None, 16, 1,
                                                     1.0, a["loss"], a["per_roi"], None, None, None)

    for kw, word in ((dict(k=1), b"classes"), (dict(k=WIDE_LIMIT + 1), b"<= 1024"), (dict(n=0), b"bad arguments"),
                     (dict(s=0), b"bad arguments"), (dict(n=1 << 20, k=64, s=64), b"2^32"),
                     (dict(n=4194304, k=1024, s=1), b"2^32"), (dict(score=None), b"null"), (dict(var=None), b"null"),
                     (dict(labels=None), b"null"), (dict(loss=None), b"null"), (dict(per_roi=None), b"null")):
        assert call(**kw) == -1 and word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())
        assert b"bayesian_cross_entropy_wide" in lib.frcnn_last_error()


# ---- on the device -------------------------------------------------------------------------------------------------
def _run_case(case_id, inp, ref, bars):
    ops = _ops()
    args = _args(inp)
    loss, dscore, dvar = ops.bayesian_cross_entropy_wide(*args, grad=BAYES_GRAD, var_is_log=inp["is_log"])
    assert bool((dvar.cpu()[inp["zero_var"]] == 0).all())                        # sd == 0: the device defines 0
    _check_all("bayes_wide", case_id, dict(loss=loss, dscore=dscore, dvar=dvar), ref, bars, "device")
    loss2, none1, none2 = ops.bayesian_cross_entropy_wide(*args, grad=BAYES_GRAD, var_is_log=inp["is_log"], want_grad=False)
    assert none1 is None and none2 is None and _bits_equal(loss, loss2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_CASES, ids=_id)
def test_wide_against_float64(hip, case):
    _run_case(_id(case), *bayes_case(*case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", NARROW_CASES, ids=_id)
def test_wide_is_bit_equal_to_the_narrow_kernel(hip, case):
    """Same expressions, same operand order of every sum: loss, dscore and dvar agree to the bit, with and without gradients
    and with the seed on the host or split between the scalar and the device word."""
    ops = _ops()
    inp, ref, bars = bayes_case(*case)
    args = _args(inp)
    kw = dict(grad=BAYES_GRAD, var_is_log=inp["is_log"])
    narrow = ops.bayesian_cross_entropy(*args, **kw)
    wide = ops.bayesian_cross_entropy_wide(*args, **kw)
    _check_all("bayes_wide", _id(case), dict(zip(("loss", "dscore", "dvar"), wide)), ref, bars, "device")
    for name, a, b in zip(("loss", "dscore", "dvar"), narrow, wide):
        assert _bits_equal(a, b), "%s differs from the narrow kernel by %.3e" % (name, float((a - b).abs().max()))
    word = torch.tensor([5], dtype=torch.int32, device=DEV)
    split = ops.bayesian_cross_entropy_wide(*(args[:4] + [BAYES_SEED - 5, BAYES_STREAM]), seed_dev=word, **kw)
    for name, a, b in zip(("loss", "dscore", "dvar"), narrow, split):
        assert _bits_equal(a, b), name + " (seed through the device word)"
    n_loss = ops.bayesian_cross_entropy(*args, want_grad=False, **kw)[0]
    w_loss, none1, none2 = ops.bayesian_cross_entropy_wide(*args, want_grad=False, **kw)
    assert none1 is None and none2 is None and _bits_equal(n_loss, w_loss) and _bits_equal(w_loss, wide[0])
    w_loss2 = ops.bayesian_cross_entropy_wide(*(args[:4] + [BAYES_SEED - 5, BAYES_STREAM]), seed_dev=word, want_grad=False,
                                              **kw)[0]
    assert _bits_equal(n_loss, w_loss2)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["logvar", "var"])
def test_planted_labels(hip, mode):
    inp, ref, bars = planted_case(mode)
    assert sorted(set(int(v) for v in inp["labels"])) == list(PLANTED)
    _run_case("planted-" + mode, inp, ref, bars)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["logvar", "var"])
def test_offset_scores(hip, mode):
    _run_case("offset-" + mode, *offset_case(mode))


@pytest.mark.gpu
def test_rows_do_not_depend_on_the_rows_after_them(hip):
    """N = 7 (N % 4 != 0): with rows 5.. replaced, rows 0..4 (a whole workgroup and the first wave of the next) keep their
    per-RoI loss and gradients bit for bit; the replaced rows change."""
    ops = _ops()
    inp, _, _ = bayes_case((7, 21, 5), "logvar")
    score, var, labels = (inp[n].clone() for n in ("score", "var", "labels"))
    g = torch.Generator().manual_seed(9)
    n0 = 5
    score2, var2, labels2 = score.clone(), var.clone(), labels.clone()
    score2[n0:] = torch.randn(7 - n0, 21, generator=g)
    var2[n0:] = torch.randn(7 - n0, 21, generator=g) * 0.5
    labels2[n0:] = (labels[n0:] + 3) % 21
    run = lambda a, b, c: ops.bayesian_cross_entropy_wide(a.to(DEV), b.to(DEV), c.to(DEV), 5, BAYES_SEED, BAYES_STREAM,
                                                          grad=BAYES_GRAD, var_is_log=True, want_per_roi=True)
    _, ds1, dv1, pr1 = run(score, var, labels)
    _, ds2, dv2, pr2 = run(score2, var2, labels2)
    assert _bits_equal(pr1[:n0], pr2[:n0]) and _bits_equal(ds1[:n0], ds2[:n0]) and _bits_equal(dv1[:n0], dv2[:n0])
    assert not bool((pr1[n0:] == pr2[n0:]).any()) and not _bits_equal(ds1[n0:], ds2[n0:])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [((3, 17, 7), "logvar"), ((6, 65, 20), "var")], ids=_id)
def test_outputs_stay_inside_guard_bands(hip, case):
    from guarded_buffers import guarded, guards_intact
    from faster_rcnn_pytorch_multimodal_amd import _hip
    ops = _ops()
    inp, _, _ = bayes_case(*case)
    (n, k, s) = case[0]
    score, var, labels = (inp[m].to(DEV) for m in ("score", "var", "labels"))
    want = ops.bayesian_cross_entropy_wide(score, var, labels, s, BAYES_SEED, BAYES_STREAM, grad=BAYES_GRAD,
                                           var_is_log=inp["is_log"], want_per_roi=True)
    bufs = [guarded(m) for m in (1, n * k, n * k, n)]                           # loss, dscore, dvar, per_roi
    (lb, lv), (sb, sv), (vb, vv), (pb, pv) = bufs
    _hip.check(hip.frcnn_bayesian_cross_entropy_wide(score.data_ptr(), var.data_ptr(), labels.data_ptr(), n, k, s, BAYES_SEED,
                                                     None, BAYES_STREAM, int(inp["is_log"]), BAYES_GRAD, lv.data_ptr(),
                                                     pv.data_ptr(), sv.data_ptr(), vv.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream),
               "frcnn_bayesian_cross_entropy_wide")
    torch.cuda.synchronize()
    for (buf, view), ref in zip(bufs, want):
        assert guards_intact(buf, view.numel())
        assert _bits_equal(view, ref.reshape(-1))                               # every element written (the fill is NaN)


@pytest.mark.gpu
def test_two_launches_and_a_captured_launch_are_bit_equal(hip):
    ops = _ops()
    inp, _, _ = bayes_case((5, 21, 200), "logvar")
    args = _args(inp)
    kw = dict(grad=BAYES_GRAD, var_is_log=True, want_per_roi=True)
    first = ops.bayesian_cross_entropy_wide(*args, **kw)
    second = ops.bayesian_cross_entropy_wide(*args, **kw)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert _bits_equal(a, b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.bayesian_cross_entropy_wide(*args, **kw)
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, captured):
            assert _bits_equal(a, b)


@pytest.mark.gpu
def test_rejections(hip):
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device=DEV)
    assert hip.frcnn_version() >= 124
    for call in (lambda: ops.bayesian_cross_entropy_wide(z(4, 1), z(4, 1), z(4), 3, 1, 16),
                 lambda: ops.bayesian_cross_entropy_wide(z(2, WIDE_LIMIT + 1), z(2, WIDE_LIMIT + 1), z(2), 3, 1, 16),
                 lambda: ops.bayesian_cross_entropy_wide(z(4, 17), z(4, 17), z(4), 0, 1, 16),
                 lambda: ops.bayesian_cross_entropy_wide(z(1024, 1024), z(1024, 1024), z(1024), 4096, 1, 16)):
        with pytest.raises(_hip_error(), match="bayesian_cross_entropy_wide"):
            call()
    with pytest.raises(_hip_error()):
        ops.bayesian_cross_entropy_wide(z(4, 17), z(4, 18), z(4), 3, 1, 16)
    with pytest.raises(_hip_error()):                                           # the narrow entry keeps its limit
        ops.bayesian_cross_entropy(z(4, 17), z(4, 17), z(4), 3, 1, 16)
