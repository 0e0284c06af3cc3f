"""The committed convolution plan table bench.py loads by default (profiles/<bench.PLANS_FILE>) under test.

Each row fixes, for one forward shape of the 1000x600 res101 frame, the tile, the split-K count, the K-steps per split and
whether the shape runs as Winograd F(2x2, 3x3) (tile code + 16) or Winograd with the input transform fused into the 64x64
GEMM's tile load (+ 32).  So this table decides which kernels the headline number times.  A row is 13 ints: the shape key
n, h, w, c, k, r, s, stride, pad, out_stride + 256 * residual, then the tile code, the splits and the steps per split.

CPU: the table's format, that every row imports and reads back, the workspace each row gets, and that rows which would drop
K-steps or leave a split empty are refused.  GPU: every row against a float64 reference at its own shape, with the dispatch
kinds proving the row's plan ran and not a fall-back; and the table is exactly the set of convolutions one frame issues.
Every test leaves the plan cache empty, the algorithm mode 0, the autotuner off and ops.PROFILE as it found it.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bench
from faster_rcnn_pytorch_multimodal_amd import _hip, ops

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PLANS_PATH = os.path.join(ROOT, "profiles", bench.PLANS_FILE)
ROWS = json.load(open(PLANS_PATH)) if os.path.exists(PLANS_PATH) else []
BK = 32                    # K-step of the implicit-GEMM kernels (conv_common.h)
RESIDUAL = 256             # key[9] flag: the call has a residual operand
DEV = "cuda:0"
INFO = np.array([0, bench.W, 0, bench.H, 0, 0, 1.0], np.float32)


def _shape(row):
    """(n, h, w, c, k, r, s, stride, pad, residual) of a row's key."""
    n, h, w, c, k, r, s, stride, pad, last = row[:10]
    return n, h, w, c, k, r, s, stride, pad, last >= RESIDUAL


def _out_hw(row):
    n, h, w, c, k, r, s, stride, pad, _ = _shape(row)
    return ops.conv_out_hw(h, w, r, s, stride, pad)


def _ksteps(row):
    n, h, w, c, k, r, s, stride, pad, _ = _shape(row)
    return -(-r * s * c // BK)


def _is_winograd(row):
    return row[10] >> 4 >= 1


def _is_fused(row):
    return row[10] >> 4 == 2


def _winograd_ws_bytes(n, h, w, c, k):
    """conv_winograd.hip wino_geom: U (16 K C) | V (16 T C) | M (16 T K) floats, each aligned to 256 bytes."""
    up = lambda v: -(-v // 256) * 256
    t = n * ((h + 1) // 2) * ((w + 1) // 2)
    return up(16 * k * c * 4) + up(16 * t * c * 4) + up(16 * t * k * 4)


def _ws_need(row):
    """The workspace a row's plan runs in: the Winograd buffers, or the split-K slabs."""
    n, h, w, c, k, r, s, stride, pad, _ = _shape(row)
    ho, wo = _out_hw(row)
    if _is_winograd(row):
        return _winograd_ws_bytes(n, h, w, c, k)
    return row[11] * n * ho * wo * k * 4 if row[11] > 1 else 0


def _row_id(row):
    n, h, w, c, k, r, s, stride, pad, res = _shape(row)
    return "%s%dx%d_%d-%d_%dx%d%s%s_t%d_s%dx%d" % ("%dx" % n if n > 1 else "", h, w, c, k, r, s,
                                                  "_str%d" % stride if stride > 1 else "", "_res" if res else "",
                                                  row[10], row[11], row[12])


def _reset():
    lib = _hip.load()
    _hip.check(lib.frcnn_conv2d_clear_plans(), "frcnn_conv2d_clear_plans")
    ops.set_conv_algo(0)
    ops.set_conv_autotune(False)


def _ws_bytes(row, split_k=0):
    n, h, w, c, k, r, s, stride, pad, _ = _shape(row)
    return int(_hip.load().frcnn_conv2d_fwd_ws_bytes(n, h, w, c, k, r, s, stride, pad, split_k))


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_plan_table_format():
    """The table bench.py loads exists, holds 13-int rows with unique keys that frcnn_conv2d_fwd can look up (output
    stride 1), and every implicit-GEMM row covers its K-steps exactly: ceil(ksteps / steps_per_split) == splits."""
    assert os.path.exists(PLANS_PATH), PLANS_PATH
    assert len(ROWS) > 0
    for row in ROWS:
        assert len(row) == 13 and all(type(v) is int for v in row), row
        assert row[9] in (1, 1 + RESIDUAL), row                     # the forward always looks up out_stride 1
        assert (row[10] & 15) < 14 and (row[10] >> 4) <= 2 and row[11] >= 1 and row[12] >= 1, row
        if _is_winograd(row):
            assert row[11] == 1 and not _shape(row)[9], row
        else:
            assert -(-_ksteps(row) // row[12]) == row[11], (row, _ksteps(row))
    keys = [tuple(r[:10]) for r in ROWS]
    assert len(set(keys)) == len(keys), "duplicate keys in %s" % bench.PLANS_FILE


def test_plan_table_imports_and_reads_back():
    """Every row imports; frcnn_conv2d_plan_algo of each key answers that row's form, and the export is the table."""
    _reset()
    try:
        ops.import_conv_plans(ROWS)
        for row in ROWS:
            n, h, w, c, k, r, s, stride, pad, res = _shape(row)
            assert ops.conv_plan_algo(n, h, w, c, k, r, s, stride, pad, res) == int(_is_winograd(row)), _row_id(row)
        assert ops.export_conv_plans() == sorted(ROWS)
    finally:
        _reset()


def test_plan_table_workspace_sizes():
    """frcnn_conv2d_fwd_ws_bytes(..., split_k = 0) with the table installed and the autotuner off: exactly the largest need of
    the cached plans of the shape (with and without a residual).  A split row thus gets its splits x M x K floats, so
    conv2d_nhwc never reaches the 'run unsplit' fall-back, and a Winograd row gets the Winograd buffers."""
    _reset()
    try:
        # the Winograd workspace formula above is the library's: forced Winograd, nothing cached, answers exactly it
        ops.set_conv_algo(2)
        for row in ROWS:
            if _is_winograd(row):
                assert _ws_bytes(row) == _ws_need(row), _row_id(row)
        ops.set_conv_algo(0)
        ops.import_conv_plans(ROWS)
        for row in ROWS:
            same_shape = [o for o in ROWS if o[:9] == row[:9]]
            got = _ws_bytes(row)
            assert got == max(_ws_need(o) for o in same_shape), (_row_id(row), got)
            if row[11] > 1:
                n, h, w, c, k = row[:5]
                ho, wo = _out_hw(row)
                assert got >= row[11] * n * ho * wo * k * 4, _row_id(row)
            if _is_winograd(row):
                assert got >= _winograd_ws_bytes(*row[:5]), _row_id(row)
    finally:
        _reset()


def _refused(rows, why):
    with pytest.raises(_hip.HipError, match=why):
        ops.import_conv_plans(rows)
    assert ops.export_conv_plans() == [], "a refused table must leave the cache as it was"


def test_plan_import_refuses_rows_that_drop_k_steps():
    """An implicit-GEMM row must split its K-steps exactly as choose_plan / the tuner do: ceil(ksteps / steps_per_split) ==
    splits.  The kernels clamp a split's range to [z * steps, min((z + 1) * steps, ksteps)), so a row that covers fewer
    K-steps would silently compute part of the convolution, and one with an empty last split hands the kernels a split
    without K-steps, which no plan the library makes contains.  A Winograd row must not split.  Rows built from real keys of
    the table; the table's own rows stay accepted."""
    gemm = [r for r in ROWS if not _is_winograd(r) and _ksteps(r) >= 4]
    wino = [r for r in ROWS if _is_winograd(r)]
    assert gemm and wino
    _reset()
    try:
        for row in gemm:
            key, tile, ks = row[:10], row[10], _ksteps(row)
            _refused([key + [tile, 1, ks - 1]], "K-steps")                       # one K-step short
            _refused([key + [tile, 1, -(-ks // 3)]], "K-steps")                  # one split's worth: 2/3 of the sum dropped
            _refused([key + [tile, 2, -(-ks // 2) - 1]], "K-steps")              # two splits, short of the sum
            _refused([key + [tile, 3, -(-ks // 2)]], "K-steps")                  # empty last split (e.g. 3 x 16 on 32)
            _refused([list(ROWS[0]), key + [tile, 1, ks - 1]], "entry 1")       # refused as a whole: nothing inserted
            ops.import_conv_plans([key + [tile, 1, ks]])                         # the unsplit plan of the same tile
            ops.import_conv_plans([row])
            assert ops.export_conv_plans() == [row]
            _reset()
        for row in wino:
            _refused([row[:11] + [2, row[12]]], "not a valid plan")
            _refused([row[:9] + [1 + RESIDUAL] + row[10:]], "not a valid plan")  # no Winograd plan for a residual call
        # the table's split rows, spelled as the issue that prompted this check: 11 of 32 K-steps
        for row in ROWS:
            if row[:10] == [1, 38, 63, 1024, 256, 1, 1, 1, 0, 1]:
                _refused([row[:10] + [row[10], 1, row[12]]], "K-steps")
    finally:
        _reset()


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _inputs(row, seed):
    n, h, w, c, k, r, s, stride, pad, res = _shape(row)
    ho, wo = _out_hw(row)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g)
    wt = torch.randn(k, r, s, c, generator=g) / np.sqrt(r * s * c)
    sc = torch.rand(k, generator=g) + 0.5
    sh = torch.randn(k, generator=g)
    rs = torch.randn(n, ho, wo, k, generator=g) if res else None
    dev = lambda t: None if t is None else t.to(DEV)
    return dev(x), dev(wt), dev(sc), dev(sh), dev(rs)


def _reference64(x, wt, sc, sh, rs, stride, pad):
    """relu(conv(x, w) * scale + shift [+ residual]) in float64 on the tensors' device: one (M x C) @ (C x K) float64 GEMM per
    filter tap, NHWC / KRSC throughout."""
    n, h, w, c = x.shape
    k, r, s, _ = wt.shape
    ho, wo = ops.conv_out_hw(h, w, r, s, stride, pad)
    xp = F.pad(x.double(), (0, 0, pad, pad, pad, pad))
    w64 = wt.double()
    y = torch.zeros(n * ho * wo, k, dtype=torch.float64, device=x.device)
    for i in range(r):
        for j in range(s):
            tap = xp[:, i:i + stride * (ho - 1) + 1:stride, j:j + stride * (wo - 1) + 1:stride, :]
            y += tap.reshape(-1, c) @ w64[:, i, j, :].t()
    y = y.view(n, ho, wo, k) * sc.double() + sh.double()
    if rs is not None:
        y = y + rs.double()
    return torch.relu(y)


def _cpu_conv64(x, wt, sc, sh, rs, stride, pad):
    y = F.conv2d(x.cpu().double().permute(0, 3, 1, 2), wt.cpu().double().permute(0, 3, 1, 2), stride=stride, padding=pad)
    y = y.permute(0, 2, 3, 1) * sc.cpu().double() + sh.cpu().double()
    if rs is not None:
        y = y + rs.cpu().double()
    return torch.relu(y)


def _expected_kinds(row, pre_filter=False):
    """Dispatch kinds frcnn_conv2d_fwd records for one call under this row's plan (launch_plan / launch_gemm /
    launch_winograd): 0 main GEMM kernel, 1 split-K second pass, 2 Winograd transform (filter unless pre-transformed, input
    unless fused, output)."""
    if _is_winograd(row):
        return [0] + [2] * (3 - int(pre_filter) - int(_is_fused(row)))
    return [0, 1] if row[11] > 1 else [0]


def _profiled(fn):
    """fn()'s result and the sorted dispatch kinds of the one frcnn_conv2d_fwd call it made."""
    ops.conv_profile_begin()
    try:
        y = fn()
    finally:
        prof = ops.conv_profile_end()
    assert {call for _, call, _ in prof} == {0}, prof
    return y, sorted(kind for _, _, kind in prof)


def _max_abs(a, b):
    return float((a.double() - b).abs().max())


@pytest.mark.gpu
def test_float64_reference_matches_cpu_conv(hip):
    """The device float64 reference of the row test below against torch's CPU float64 convolution: on the table's smallest
    row as it stands, and on small maps with each filter geometry (r, s, stride, pad) of the table, with and without a residual."""
    smallest = min(ROWS, key=lambda r: np.prod(r[:5], dtype=np.int64) * r[5] * r[6] // r[7] ** 2)
    cases = [smallest]
    for r_, s_, stride, pad, res in sorted({tuple(r[5:9]) + (_shape(r)[9],) for r in ROWS}):
        cases.append([2, 9, 11, 8, 12, r_, s_, stride, pad, 1 + RESIDUAL * res, 5, 1, 1])
    for row in cases:
        n, h, w, c, k, r, s, stride, pad, res = _shape(row)
        x, wt, sc, sh, rs = _inputs(row, 7 + sum(row[:10]))
        ref = _reference64(x, wt, sc, sh, rs, stride, pad).cpu()
        cpu = _cpu_conv64(x, wt, sc, sh, rs, stride, pad)
        assert ref.shape == cpu.shape
        assert float((ref - cpu).abs().max()) <= 1e-12 * float(cpu.abs().max()), _row_id(row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[_row_id(r) for r in ROWS])
def test_plan_table_row_against_float64(hip, row):
    """One row of the committed table, installed alone, through conv2d_nhwc(split_k = 0) - the path that uses cached plans -
    against float64 over the whole output.  The dispatch kinds prove that the row's plan ran (split-K second pass iff split,
    Winograd transforms iff Winograd, one fewer when fused or pre-transformed) and not a fall-back.  Bars: those of
    test_conv2d_fwd (implicit GEMM: 1e-5 of max |ref|) and test_conv2d_winograd_matches_direct_and_float64 (Winograd:
    within 3x the direct form's float64 error or 2e-6 of the scale, and 1e-5 of the scale from the direct form)."""
    n, h, w, c, k, r, s, stride, pad, res = _shape(row)
    x, wt, sc, sh, rs = _inputs(row, 1000 + sum(row))
    ref = _reference64(x, wt, sc, sh, rs, stride, pad)
    scale = float(ref.abs().max())
    run = lambda **kw: ops.conv2d_nhwc(x, wt, sc, sh, rs, stride=stride, pad=pad, relu=True, split_k=0, **kw)
    _reset()
    try:
        ops.import_conv_plans([row])
        got, kinds = _profiled(run)
        assert kinds == _expected_kinds(row), "%s: dispatch kinds %s, the plan's are %s" % (_row_id(row), kinds,
                                                                                          _expected_kinds(row))
        again = run()
        assert torch.equal(got, again), "%s: not deterministic" % _row_id(row)
        err = _max_abs(got, ref)
        print("%s: max |err| vs float64 %.3g, scale %.3g" % (_row_id(row), err, scale))
        if _is_winograd(row):
            u = ops.winograd_filter(wt)
            pre, kinds_pre = _profiled(lambda: run(w_winograd=u))
            assert kinds_pre == _expected_kinds(row, pre_filter=True), (_row_id(row), kinds_pre)
            assert torch.equal(got, pre), "%s: frcnn_conv2d_fwd_pre differs from frcnn_conv2d_fwd" % _row_id(row)
            _reset()
            ops.set_conv_algo(1)
            direct = run()
            err_d = _max_abs(direct, ref)
            print("%s: direct form max |err| vs float64 %.3g" % (_row_id(row), err_d))
            assert err <= max(3.0 * err_d, 2e-6 * scale), (_row_id(row), err, err_d, scale)
            assert float((got - direct).abs().max()) <= 1e-5 * scale, _row_id(row)
        else:
            assert err <= 1e-5 * scale, "%s: max abs err %.3e > %.3e" % (_row_id(row), err, 1e-5 * scale)
            if row[11] > 1:                           # the same tile unsplit
                _reset()
                ops.import_conv_plans([row[:11] + [1, _ksteps(row)]])
                unsplit, kinds_u = _profiled(run)
                assert kinds_u == [0], (_row_id(row), kinds_u)
                assert _max_abs(unsplit, ref) <= 1e-5 * scale, _row_id(row)
                assert float((got - unsplit).abs().max()) <= 1e-5 * scale, _row_id(row)
    finally:
        _reset()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_plan_table_is_exactly_the_frames_convolutions(hip):
    """With the table installed, one eager frame of bench.py's runner (its arguments, minus the graph; autotune on as bench
    has it) issues exactly the table's keys - no stale row, no untabled shape - and tunes nothing: the export afterwards is the
    table.  Every convolution goes through conv2d_nhwc, so ops.PROFILE sees them all.  Together with the row test above this
    says that the kernels bench.py times are the ones checked against float64."""
    from faster_rcnn_pytorch_multimodal_amd.model.frame_graph import FrameRunner
    saved_profile = ops.PROFILE
    _reset()
    try:
        ops.import_conv_plans(ROWS)
        ops.PROFILE = []
        net, _ = bench.build_net(DEV)
        FrameRunner(net, bench.H, bench.W, bench.C, INFO, bench.THRESH, bench.MAX_DETS, use_graph=False, autotune=True)
        torch.cuda.synchronize()
        issued = {(p["n"], p["h"], p["w"], p["c"], p["k"], p["r"], p["s"], p["stride"], p["pad"], 1 + RESIDUAL * p["residual"])
                  for p in ops.PROFILE}
        exported = ops.export_conv_plans()
    finally:
        ops.PROFILE = saved_profile
        _reset()
    table = {tuple(r[:10]) for r in ROWS}
    assert not table - issued, "rows of %s the frame never issues: %s" % (bench.PLANS_FILE, sorted(table - issued))
    assert not issued - table, "convolutions of the frame without a row in %s: %s" % (bench.PLANS_FILE, sorted(issued - table))
    assert exported == sorted(ROWS), "the frame tuned plans beyond the table: %s" % [r for r in exported if r not in ROWS]
