"""NaN and Inf survive the feature path: every kernel that carries activations or their gradients, with one non-finite value
placed in one operand, against torch on the host ("Non-finite values on the feature path").

The rule.  The reference runs nn.ReLU, nn.ReLU6, nn.MaxPool2d and train-mode BatchNorm: relu(NaN) is NaN, a pooling window that
holds a NaN gives NaN (NaN beats +inf), and the backward masks are ``x <= 0 ? 0 : g`` - open where the activation is NaN.  So
a NaN weight or an overflowed activation turns the reference's loss NaN at once.  fmaxf / fminf / ``v > 0 ? v : 0`` erase it.

One table of cases (CASES): a kernel form, the poisoned operand, the poison.  Each case runs the device twice, clean (C) and
poisoned (P), and has one reference R: the same operation on the poisoned operands with torch on the host, in float64 (float32
for the pools, the clamp and the activation masks, whose existing tests use float32 torch).  ``judge`` asserts:

  1. nothing is erased: isnan(P) covers isnan(R); where R is +-inf, P is not finite.  For the kernels whose arithmetic is
     element for element the reference's ("exact": the implicit-GEMM fp32 forms, the pools, the BatchNorm apply, the depthwise
     convolution, the activation kernels) the NaN positions are EQUAL and P == R at the Inf positions - and, the operands being
     small integers (tests/test_conv_f32_exact.py), at every finite position too.
  2. nothing else is touched: outside the footprint of the poison P equals C bit for bit.  The footprint is ~isfinite(R)
     together with the elements whose finite reference value the poison changed (a -inf behind the ReLU is an exact 0 where
     the clean run is positive) ("exact"), its closure over 2x2 output tiles (Winograd, "tiled"), the whole channel (train-mode BatchNorm).  The
     bf16-operand and split-bf16 forms document that an infinite operand gives NaN (ops.conv2d_nhwc_bf16x3): rule 1 only
     ("superset").
  3. the case is not vacuous (``host_check``, in the unmarked test_cpu_reference_* tests, before any device run): R holds a
     NaN or Inf BEHIND the ReLU / pool / mask, where fmaxf would have erased it, and a finite element.

Operands hold no exact zero next to the poison (x, w, dy are integers of [-3, 3] without 0), so 0 * NaN decides nothing; a
poisoned filter tap is the centre tap, which lies inside the map for every output.

Buffers.  Where the wrapper takes ``out=`` (the convolutions, maxpool2x2, the depthwise kernels) or the C entry point is called
directly (maxpool3x3), the output is a view between NaN guard bands (tests/guarded_buffers.py), pre-filled with a FINITE
sentinel, so a NaN in it proves a write; the bands must stay NaN.  bn_train_*, act_bwd and the plain-arithmetic wrappers
allocate their own outputs.

The forward entry point admits K % 4 != 0 (conv_args_ok asks only C % 4 == 0), so the element-wise epilogue has a case (k6).
"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import test_batchnorm_kernels as BN
import test_conv_f32_exact as E
from guarded_buffers import DEV, guarded, guards_flag
from test_resample_gather_kernels import POOL_MAPS

NAN, INF = float("nan"), float("inf")
KINDS = {"nan": NAN, "+inf": INF, "-inf": -INF}
SENTINEL = -77.25
BAND = E.BAND
U = 2.0 ** -23

SHAPES = dict(E.SHAPES, k6=(1, 3, 5, 32, 6, 1, 1, 0))        # K % 4 != 0: the element-wise store path of conv_epilogue
assert (7, 8) in POOL_MAPS and (1, 9) in POOL_MAPS


def _ops():
    from faster_rcnn_pytorch_multimodal_amd import ops
    return ops


# ---- the verdict -----------------------------------------------------------------------------------------------------------------
def host_check(label, R, behind=None):
    """Rule 3: R holds a non-finite value (inside ``behind``, a mask of the elements behind the ReLU / pool, when given) and a
    finite one."""
    bad = ~torch.isfinite(R)
    assert bool((bad if behind is None else bad & behind).any()), "%s: the reference carries nothing non-finite to assert on" % label
    assert bool((~bad).any()), "%s: the reference holds no finite element" % label
    return True


def tile_closure(mask):
    """(n, h, w, k) bool -> its closure over the 2x2 output tiles of F(2x2, 3x3)."""
    n, h, w, k = mask.shape
    t = F.max_pool2d(mask.permute(0, 3, 1, 2).float(), 2, 2, ceil_mode=True)
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :h, :w].permute(0, 2, 3, 1).bool()


def _bits(t):
    return t.contiguous().view(torch.int32)


def judge(label, P, C, R, rule="exact", footprint=None, values=False, R0=None):
    """Rules 1 and 2 of the module docstring.  ``values``: P == R at every finite position of R as well (integer operands).
    ``R0``: the reference on the clean operands - the footprint then also holds the elements whose FINITE reference value the
    poison changed (relu(-inf) = 0 where the clean run is positive)."""
    P, C = P.detach().cpu().reshape(R.shape), C.detach().cpu().reshape(R.shape)
    assert bool(torch.isfinite(C).all()), "%s: the clean run is not finite" % label
    rn, pn, ri = torch.isnan(R), torch.isnan(P), torch.isinf(R)
    erased = (rn & ~pn) | (ri & torch.isfinite(P))
    assert not bool(erased.any()), "%s: %d non-finite reference values were erased, first at %s: got %r, want %r" % (
        label, int(erased.sum()), erased.nonzero()[0].tolist(), float(P[erased][0]), float(R[erased][0]))
    if rule == "superset":
        return
    if footprint is None:
        footprint = ~torch.isfinite(R)
        if R0 is not None:
            footprint = footprint | (R.double() != R0.double())
        if rule == "tiled":
            footprint = tile_closure(footprint)
    if rule == "exact":
        assert torch.equal(pn, rn), "%s: NaN positions differ from the reference's" % label
        assert bool((P.double()[ri] == R.double()[ri]).all()), "%s: an infinity differs from the reference's" % label
        if values:
            assert bool(((P.double() == R.double()) | rn).all()), "%s: a finite value differs from the reference's" % label
    outside = ~footprint
    assert torch.equal(_bits(P)[outside], _bits(C)[outside]), "%s: %d elements outside the poison's footprint changed" % (
        label, int((_bits(P) != _bits(C))[outside].sum()))


def out_view(shape):
    numel = 1
    for s in shape:
        numel *= s
    buf, view = guarded(numel, fill=SENTINEL, guard=BAND)
    return buf, view.view(*shape)


def bands_intact(label, buf, view):
    assert bool(guards_flag(buf, view.numel(), BAND)), "%s: wrote outside the output" % label


def poison(t, index, kind):
    t = t.clone()
    t[index] = KINDS[kind]
    return t


# ---- torch's own behaviour, pinned -------------------------------------------------------------------------------------------------
def test_cpu_reference_torch_facts():
    """What the kernels follow: a torch upgrade that changes one of these must be noticed here, not in a diverged training."""
    x = torch.tensor([NAN, -1.0, 0.0, 2.0, INF, -INF], requires_grad=True)
    y = F.relu(x)
    assert torch.isnan(y[0]) and y[1:].tolist() == [0.0, 0.0, 2.0, INF, 0.0]
    y.backward(torch.full_like(x, 3.0))
    assert x.grad.tolist() == [3.0, 0.0, 0.0, 3.0, 3.0, 0.0]              # x <= 0 ? 0 : g - open for the NaN
    x6 = torch.tensor([NAN, -1.0, 0.0, 2.0, 6.0, INF], requires_grad=True)
    y6 = F.relu6(x6)
    assert torch.isnan(y6[0]) and y6[1:].tolist() == [0.0, 0.0, 2.0, 6.0, 6.0]
    y6.backward(torch.full_like(x6, 3.0))
    # closed at both ends, open for the NaN.  (Six elements: below a vector width, so the host's scalar loop answers - its
    # vectorised hardtanh_backward loop gives 0 for a NaN in torch 2.10, unlike the scalar loop and the device kernel.)
    assert x6.grad.tolist() == [3.0, 0.0, 0.0, 3.0, 0.0, 0.0]
    assert torch.isnan(torch.clamp(torch.tensor([NAN]), max=6.0)).all()
    m = torch.tensor([[1.0, INF, 2.0], [3.0, NAN, 4.0], [5.0, 6.0, NAN]], requires_grad=True)
    p, idx = F.max_pool2d(m[None, None], 3, 2, 1, return_indices=True)
    assert torch.isnan(p[0, 0, 0, 0]) and int(idx[0, 0, 0, 0]) == 4        # window rows 0..1, cols 0..1: NaN beats +inf
    assert torch.isnan(p[0, 0, 1, 1]) and int(idx[0, 0, 1, 1]) == 8        # two NaN in the window: the last one
    p.backward(torch.ones_like(p))
    assert bool(torch.isfinite(m.grad).all()) and float(m.grad[1, 1]) >= 1.0 and float(m.grad[2, 2]) == 1.0
    b = torch.randn(6, 3, dtype=torch.float64)
    b[2, 1] = NAN
    o = F.relu(F.batch_norm(b, None, None, torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), True, 0.1, 1e-5))
    assert bool(torch.isnan(o[:, 1]).all()) and bool(torch.isfinite(o[:, [0, 2]]).all())


# ================================================================================================
# 1. forward convolutions
# ================================================================================================
# form -> shape, hooks, rule.  plan = (tile index, splits, K-steps per split or None for all)
FWD_FORMS = {
    "igemm_lds_epilogue": dict(shape="m65_c36_k68", algo=1),                        # conv_epilogue_lds (register-staged, unaligned C)
    "igemm_mfma_store": dict(shape="m65_c36_k68", algo=1 | 64),                     # conv_epilogue, the aligned 16-byte stores
    "igemm_elementwise_k6": dict(shape="k6", algo=1),                               # conv_epilogue, K % 4 != 0
    "split_k_epilogue": dict(shape="k260_3steps", algo=1, plan=(5, 2, 2)),          # conv_splitk_epilogue
    "buffer_load_tile": dict(shape="m259_k132", algo=1, plan=(7, 1, None), staging=1),
    "persistent_tile": dict(shape="m259_k132", algo=1, plan=(13, 1, None), staging=1),
    "winograd_separate": dict(shape="3x3_odd_batch", algo=2 | 16, rule="tiled"),
    "winograd_fused": dict(shape="3x3_odd_batch", algo=2 | 32, rule="tiled"),
    "bf16": dict(shape="m259_k132", entry="bf16", rule="superset"),
    "bf16x3": dict(shape="m259_k132", entry="bf16x3", rule="superset"),
}
FWD_POISONS = [("x", "nan"), ("x", "+inf"), ("x", "-inf"), ("w", "nan"), ("w", "+inf"), ("scale", "nan"), ("shift", "nan"),
               ("shift", "+inf"), ("residual", "nan"), ("residual", "+inf")]


def _fwd_cases():
    cases = []
    for form, spec in FWD_FORMS.items():
        wino = spec.get("rule") == "tiled"                          # a residual under forced Winograd runs the implicit GEMM
        for operand, kind in FWD_POISONS:
            if wino and operand == "residual":
                continue
            cases.append((form, "scale_shift_relu" if wino else "scale_shift_residual_relu", operand, kind))
        if not wino:
            cases.append((form, "scale_shift_relu", "x", "nan"))
    return cases


FWD_CASES = _fwd_cases()


@functools.lru_cache(maxsize=None)
def conv_operands(name):
    """test_conv_f32_exact's operand ranges (its exactness argument holds) without an exact zero in x, w, dy."""
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = E.out_hw(h, w, r, stride, pad)
    gen = torch.Generator().manual_seed(7000 + list(SHAPES).index(name))
    ints = lambda *shape: torch.randint(-3, 4, shape, generator=gen).double()
    nz = lambda t: torch.where(t == 0, torch.ones_like(t), t)
    pow2 = lambda count: torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (count,), generator=gen)]
    return {"x": nz(ints(n, h, w, c)), "w": nz(ints(k, r, r, c)), "dy": nz(ints(n, ho, wo, k)), "residual": ints(n, ho, wo, k),
            "add": ints(n, h, w, c), "scale": pow2(k), "shift": ints(k), "act_scale": pow2(c),
            "act_y": torch.randn((n, h, w, c), generator=gen, dtype=torch.float32).clamp_min(0).double()}


def poison_index(name, operand):
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = E.out_hw(h, w, r, stride, pad)
    return {"x": (n - 1, h // 2, w // 2, c - 3), "w": (k - 1, r // 2, r // 2, c - 3), "scale": (k - 1,), "shift": (k - 1,),
            "residual": (n - 1, ho // 2, wo // 2, k - 1), "dy": (n - 1, ho // 2, wo // 2, k - 1), "add": (n - 1, h // 2, w // 2, c - 3),
            "act_scale": (c - 3,)}[operand]


def fwd_float64(name, t, epilogue, relu=True):
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    y = F.conv2d(t["x"].permute(0, 3, 1, 2), t["w"].permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1)
    y = y * t["scale"] + t["shift"]
    y = (y + t["residual"] if epilogue == "scale_shift_residual_relu" else y).contiguous()
    return torch.relu(y) if relu else y


@functools.lru_cache(maxsize=None)
def fwd_reference(name, epilogue, operand, kind):
    t = dict(conv_operands(name))
    t[operand] = poison(t[operand], poison_index(name, operand), kind)
    return t, fwd_float64(name, t, epilogue)


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "-".join(c))
def test_cpu_reference_forward_conv(case):
    form, epilogue, operand, kind = case
    name = FWD_FORMS[form]["shape"]
    assert E.exact_regime(name) if name in E.SHAPES else name == "k6"
    _, R = fwd_reference(name, epilogue, operand, kind)                    # every element of R lies behind the ReLU
    assert host_check("-".join(case), R)
    assert bool(torch.isfinite(fwd_float64(name, conv_operands(name), epilogue)).all())


@contextlib.contextmanager
def fwd_hooks(spec):
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k, r, stride, pad = SHAPES[spec["shape"]]
    with E.hooks():
        if "plan" in spec:
            idx, splits, per_split = spec["plan"]
            key = [n, h, w, c, k, r, r, stride, pad]
            row = [idx, splits, per_split or (r * r * c + 31) // 32]
            E.import_plans([key + [1] + row, key + [1 + 256] + row])
            assert sorted(r_[9:] for r_ in ops.export_conv_plans()) == [[1] + row, [1 + 256] + row], "the plan rows did not take"
        if "staging" in spec:
            E.set_staging(spec["staging"])
        if "algo" in spec:
            ops.set_conv_algo(spec["algo"])
        yield


_FWD_DEVICE = {}


def run_forward(form, epilogue, t):
    """One guarded launch of the form on host operands ``t``; returns the output on the host."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    spec = FWD_FORMS[form]
    n, h, w, c, k, r, stride, pad = SHAPES[spec["shape"]]
    ho, wo = E.out_hw(h, w, r, stride, pad)
    d = {key: t[key].float().to(DEV).contiguous() for key in ("x", "w", "scale", "shift", "residual")}
    res = d["residual"] if epilogue == "scale_shift_residual_relu" else None
    obuf, out = out_view((n, ho, wo, k))
    entry = spec.get("entry")
    if entry:
        pack, conv = (ops.conv2d_pack_bf16, ops.conv2d_nhwc_bf16) if entry == "bf16" else (ops.conv2d_pack_bf16x3, ops.conv2d_nhwc_bf16x3)
        conv(d["x"], pack(d["w"]), d["scale"], d["shift"], res, stride=stride, pad=pad, relu=True, out=out)
    else:
        with fwd_hooks(spec):
            ws_floats = E.floats_of(int(E.lib().frcnn_conv2d_fwd_ws_bytes(n, h, w, c, k, r, r, stride, pad, 0)))
            if "plan" in spec and spec["plan"][1] > 1:
                assert ws_floats >= spec["plan"][1] * n * ho * wo * k, "the split-K plan row did not take"
            wbuf, ws = guarded(ws_floats, guard=BAND)
            ops.conv2d_nhwc(d["x"], d["w"], d["scale"], d["shift"], res, stride=stride, pad=pad, relu=True, out=out, ws=ws)
            assert bool(guards_flag(wbuf, ws_floats, BAND)), "%s: wrote outside the workspace" % form
    bands_intact(form, obuf, out)
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "-".join(c))
def test_forward_conv_carries_the_poison(hip, case):
    form, epilogue, operand, kind = case
    spec = FWD_FORMS[form]
    name = spec["shape"]
    t, R = fwd_reference(name, epilogue, operand, kind)
    if (form, epilogue) not in _FWD_DEVICE:
        _FWD_DEVICE[(form, epilogue)] = run_forward(form, epilogue, conv_operands(name))
    C = _FWD_DEVICE[(form, epilogue)]
    rule = spec.get("rule", "exact")
    if rule != "superset":                                           # integer operands: the clean run is the float64 result
        assert torch.equal(C.double(), fwd_float64(name, conv_operands(name), epilogue))
    # the footprint is taken in front of the ReLU: a -inf that it turns into the 0 the clean run holds as well is still an
    # element the poison reached (Winograd: inf - inf inside the tile's transforms may leave a NaN there)
    footprint = ~torch.isfinite(fwd_float64(name, t, epilogue, relu=False))
    judge("-".join(case), run_forward(form, epilogue, t), C, R, rule, values=True,
          footprint=tile_closure(footprint) if rule == "tiled" else footprint)


# ================================================================================================
# 2. data gradient with the activation epilogue (add, act_y, act_scale)
# ================================================================================================
# dgrad plans are keyed by the forward convolution the gradient runs as: (n, ho, wo, K -> C, r, r, 1, r - 1 - pad)
DGRAD_FORMS = {
    "igemm": dict(shape="m65_c36_k68", algo=1, add=True),
    "split_k_epilogue": dict(shape="k260_3steps", algo=1, add=True, plan=(5, 2, 5)),    # 9 K-steps of dy's 260 channels
    "winograd": dict(shape="3x3_odd_batch", algo=2, add=False, rule="tiled"),
    "bf16": dict(shape="3x3_odd_batch", entry="bf16", add=True, rule="superset"),
}
DGRAD_POISONS = [("dy", "nan"), ("dy", "+inf"), ("dy", "-inf"), ("add", "nan"), ("act_scale", "nan"), ("act_y", "nan")]
DGRAD_CASES = [(form, operand, kind) for form, spec in DGRAD_FORMS.items() for operand, kind in DGRAD_POISONS
               if spec["add"] or operand != "add"]


def dgrad_float64(name, t, add):
    """torch's rule for the mask: y <= 0 ? 0 : g."""
    v = E.dx_float64(name, t["dy"], t["w"])
    v = (v + t["add"] if add else v) * t["act_scale"]
    return torch.where(t["act_y"] <= 0, torch.zeros_like(v), v)


def act_y_index(name, add):
    """A closed mask element whose gradient is not 0 behind it: a NaN there must open it."""
    t = conv_operands(name)
    v = E.dx_float64(name, t["dy"], t["w"]) + (t["add"] if add else 0)
    at = ((t["act_y"] == 0) & (v != 0)).nonzero()
    return tuple(at[len(at) // 2].tolist())


def open_index(name):
    """An open mask element, for the poisoned `add`: behind a closed one torch's gradient is 0 whatever is added."""
    at = (conv_operands(name)["act_y"] > 0).nonzero()
    return tuple(at[len(at) // 2].tolist())


@functools.lru_cache(maxsize=None)
def dgrad_reference(name, add, operand, kind):
    t = dict(conv_operands(name))
    index = {"act_y": lambda: act_y_index(name, add), "add": lambda: open_index(name)}.get(operand, lambda: poison_index(name, operand))()
    t[operand] = poison(t[operand], index, kind)
    return t, dgrad_float64(name, t, add)


@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "-".join(c))
def test_cpu_reference_data_gradient(case):
    form, operand, kind = case
    spec = DGRAD_FORMS[form]
    name = spec["shape"]
    assert E.exact_regime(name)
    _, R = dgrad_reference(name, spec["add"], operand, kind)
    clean = dgrad_float64(name, conv_operands(name), spec["add"])
    assert bool(torch.isfinite(clean).all())
    if operand == "act_y":                                           # the NaN opens the mask: a gradient where the clean run has 0
        at = act_y_index(name, spec["add"])
        assert float(clean[at]) == 0.0 and float(R[at]) != 0.0 and bool(torch.isfinite(R).all())
        assert int((R != clean).sum()) == 1
    else:
        assert host_check("-".join(case), R, behind=conv_operands(name)["act_y"] > 0)
        if operand == "dy":                                          # and the closed mask elements inside the window stay 0
            window = ~torch.isfinite(E.dx_float64(name, dgrad_reference(name, spec["add"], operand, kind)[0]["dy"], conv_operands(name)["w"]))
            assert bool((window & (R == 0)).any())


_DGRAD_DEVICE = {}


def run_dgrad(form, t):
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    spec = DGRAD_FORMS[form]
    name = spec["shape"]
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = E.out_hw(h, w, r, stride, pad)
    d = {key: t[key].float().to(DEV).contiguous() for key in ("dy", "w", "add", "act_y", "act_scale")}
    w_t = ops.conv2d_transpose_filter(d["w"])
    add = d["add"] if spec["add"] else None
    obuf, out = out_view((n, h, w, c))
    if spec.get("entry") == "bf16":
        ws_floats = max((int(_hip.load().frcnn_conv2d_bwd_data_bf16_ws_bytes(n, h, w, c, k, r, r, stride, pad)) + 3) // 4, 4)
        wbuf, ws = guarded(ws_floats, guard=BAND)
        ops.conv2d_bwd_data_bf16(d["dy"], ops.conv2d_pack_bf16(w_t), (n, h, w, c), stride=stride, pad=pad, add=add, act_y=d["act_y"],
                                 act_scale=d["act_scale"], out=out, ws=ws)
    else:
        with E.hooks():
            if "plan" in spec:
                idx, splits, per_split = spec["plan"]
                key = [n, ho, wo, k, c, r, r, 1, r - 1 - pad]
                E.import_plans([key + [1, idx, splits, per_split], key + [1 + 256, idx, splits, per_split]])
            ops.set_conv_algo(spec["algo"])
            ws_floats = E.floats_of(int(E.lib().frcnn_conv2d_bwd_data_ws_bytes(n, h, w, c, k, r, r, stride, pad)))
            if "plan" in spec:
                assert ws_floats >= spec["plan"][1] * n * h * w * c, "the split-K plan row did not take"
            wbuf, ws = guarded(ws_floats, guard=BAND)
            ops.conv2d_bwd_data(d["dy"], w_t, (n, h, w, c), stride=stride, pad=pad, add=add, act_y=d["act_y"], act_scale=d["act_scale"],
                                out=out, ws=ws)
    assert bool(guards_flag(wbuf, ws_floats, BAND)), "%s: wrote outside the workspace" % form
    bands_intact(form, obuf, out)
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "-".join(c))
def test_data_gradient_carries_the_poison(hip, case):
    form, operand, kind = case
    spec = DGRAD_FORMS[form]
    name = spec["shape"]
    t, R = dgrad_reference(name, spec["add"], operand, kind)
    if form not in _DGRAD_DEVICE:
        _DGRAD_DEVICE[form] = run_dgrad(form, conv_operands(name))
    C, P = _DGRAD_DEVICE[form], run_dgrad(form, t)
    rule = spec.get("rule", "exact")
    if operand == "act_y":
        at = act_y_index(name, spec["add"])
        assert float(C[at]) == 0.0
        if rule == "superset":                                       # products of bf16-rounded operands: integers of [-3, 3] are exact
            assert float(P[at]) != 0.0 and bool(torch.isfinite(P).all())
        else:
            assert float(P[at]) == float(R[at]), "%s: a NaN activation must open the mask (torch: y <= 0 ? 0 : g)" % form
        opened = torch.zeros(R.shape, dtype=torch.bool)
        opened[at] = True
        assert torch.equal(_bits(P)[~opened], _bits(C)[~opened])
        return
    judge("-".join(case), P, C, R, rule, values=True, R0=dgrad_float64(name, conv_operands(name), spec["add"]))


# ================================================================================================
# 3. filter gradient
# ================================================================================================
WGRAD_SHAPE = "m259_k132"
WGRAD_FORMS = [("register_staged", 1, 1), ("register_staged", 1, 3), ("lds_dma", 3, 1), ("lds_dma", 3, 3), ("bf16", 0, 0)]
WGRAD_CASES = [(family, kernel, splits, kind) for family, kernel, splits in WGRAD_FORMS for kind in ("nan", "+inf")]


@functools.lru_cache(maxsize=None)
def wgrad_reference(kind):
    t = dict(conv_operands(WGRAD_SHAPE))
    if kind:
        t["dy"] = poison(t["dy"], poison_index(WGRAD_SHAPE, "dy"), kind)
    return t, E.dw_float64(WGRAD_SHAPE, t["x"], t["dy"]), t["dy"].reshape(-1, t["dy"].shape[-1]).sum(0)


@pytest.mark.parametrize("kind", ["nan", "+inf"])
def test_cpu_reference_filter_gradient(kind):
    """One poisoned dy element: every tap of its output channel's dw and its db are non-finite, every other channel is the
    clean gradient."""
    k0 = poison_index(WGRAD_SHAPE, "dy")[-1]
    _, dw, db = wgrad_reference(kind)
    _, dw0, db0 = wgrad_reference(None)
    others = torch.arange(dw.shape[0]) != k0
    assert not bool(torch.isfinite(dw[k0]).any()) and not bool(torch.isfinite(db[k0]))
    assert torch.equal(dw[others], dw0[others]) and torch.equal(db[others], db0[others]) and bool(torch.isfinite(dw0).all())


def run_wgrad(kernel, splits, t):
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k, r, stride, pad = SHAPES[WGRAD_SHAPE]
    x, dy = t["x"].float().to(DEV), t["dy"].float().to(DEV)
    obuf, out = out_view((k, r, r, c))
    if kernel == 0:
        dw, db = ops.conv2d_bwd_weight_bf16(x, dy, r, r, stride=stride, pad=pad, want_bias=True, out=out)
    else:
        with E.hooks():
            ops.set_wgrad_plan(kernel, splits)
            ws_floats = E.floats_of(int(E.lib().frcnn_conv2d_bwd_weight_ws_bytes(n, h, w, c, k, r, r, stride, pad)))
            wbuf, ws = guarded(ws_floats, guard=BAND)
            bbuf, bias = out_view((k,))
            dw, db = ops.conv2d_bwd_weight(x, dy, r, r, stride=stride, pad=pad, want_bias=True, out=out, out_bias=bias, ws=ws)
            assert bool(guards_flag(wbuf, ws_floats, BAND)) and bool(guards_flag(bbuf, k, BAND))
    bands_intact("filter gradient", obuf, out)
    torch.cuda.synchronize()
    for ring in ops._COUNTER_RINGS.values():
        assert int(ring.ints.abs().max()) == 0, "tile counters are not zero again"
    return dw.cpu(), db.cpu()


_WGRAD_DEVICE = {}


@pytest.mark.gpu
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "%s-k%d-s%d-%s" % c)
def test_filter_gradient_carries_the_poison(hip, case):
    family, kernel, splits, kind = case
    k0 = poison_index(WGRAD_SHAPE, "dy")[-1]
    t, dw_ref, db_ref = wgrad_reference(kind)
    if (kernel, splits) not in _WGRAD_DEVICE:
        _WGRAD_DEVICE[(kernel, splits)] = run_wgrad(kernel, splits, wgrad_reference(None)[0])
    (dw0, db0), (dw, db) = _WGRAD_DEVICE[(kernel, splits)], run_wgrad(kernel, splits, t)
    rule = "superset" if family == "bf16" else "exact"
    channel = torch.zeros(dw_ref.shape, dtype=torch.bool)
    channel[k0] = True
    judge("dw %s" % (case,), dw, dw0, dw_ref, rule, footprint=channel, values=True)
    judge("db %s" % (case,), db, db0, db_ref, rule, footprint=channel[:, 0, 0, 0], values=True)
    assert torch.equal(_bits(dw)[~channel], _bits(dw0)[~channel])     # (the bf16 form too: every other channel keeps its bits)
    assert not bool(torch.isfinite(dw[k0]).any()) and not bool(torch.isfinite(db[k0]))


# ================================================================================================
# 4. max-pools
# ================================================================================================
POOL3_PATTERNS = ["nan_alone", "nan_next_to_inf", "two_nans", "nan_in_the_corner", "inf_alone"]
POOL3_CASES = [(hw, p) for hw in ((7, 8), (1, 9)) for p in POOL3_PATTERNS]
POOL_C = 8
POOL_CH = 5                                                           # the poisoned channel: second float4 of the pixel


@functools.lru_cache(maxsize=None)
def pool3_case(hw, pattern):
    """(clean x, poisoned x, dy, R forward, R backward, torch's indices) - float32 torch, as tests/test_resample_gather_kernels.py."""
    h, w = hw
    g = torch.Generator().manual_seed(900 + h * 16 + w)
    x = torch.randn((2, h, w, POOL_C), generator=g)
    a, b = ((3, 4), (4, 5)) if h > 1 else ((0, 4), (0, 5))
    xp = x.clone()
    if pattern == "nan_in_the_corner":
        xp[0, 0, 0, POOL_CH] = NAN
    elif pattern == "inf_alone":
        xp[1, a[0], a[1], POOL_CH] = INF
    else:
        xp[1, a[0], a[1], POOL_CH] = NAN
        if pattern == "nan_next_to_inf":
            xp[1, a[0], a[1] + 1, POOL_CH] = INF
        if pattern == "two_nans":
            xp[1, b[0], b[1], POOL_CH] = NAN
    xr = xp.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y, idx = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return x, xp, nhwc(dy), nhwc(y), nhwc(xr.grad), idx


@pytest.mark.parametrize("case", POOL3_CASES, ids=lambda c: "%dx%d-%s" % (c[0] + (c[1],)))
def test_cpu_reference_maxpool3x3(case):
    x, xp, dy, R, Rb, idx = pool3_case(*case)
    assert host_check(str(case), R) and bool(torch.isfinite(R[..., [c for c in range(POOL_C) if c != POOL_CH]]).all())
    if case[1] != "inf_alone":
        holds = F.max_pool2d(torch.isnan(xp).permute(0, 3, 1, 2).float(), 3, 2, 1).permute(0, 2, 3, 1) > 0
        assert torch.equal(torch.isnan(R), holds) and bool(holds.any())               # every window that holds a NaN: NaN beats +inf
        # a window that holds a NaN names one as its winner, and that pixel receives the window's dy: finite gradients on NaN pixels
        flat = xp.permute(0, 3, 1, 2).reshape(2, POOL_C, -1)
        winners = torch.gather(flat, 2, idx.reshape(2, POOL_C, -1))
        assert torch.equal(torch.isnan(winners), torch.isnan(R.permute(0, 3, 1, 2).reshape(2, POOL_C, -1)))
        assert bool(torch.isfinite(Rb).all()) and bool((Rb[torch.isnan(xp)] != 0).any())


def pool3_device(x, dy=None):
    """frcnn_maxpool3x3s2_fwd / _bwd through the C ABI, into guarded views (the wrappers allocate their own output)."""
    lib = E.lib()
    n, h, w, c = x.shape
    xd = x.to(DEV).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    if dy is None:
        buf, out = out_view((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c))
        assert lib.frcnn_maxpool3x3s2_fwd(xd.data_ptr(), out.data_ptr(), n, h, w, c, stream) == 0
    else:
        buf, out = out_view((n, h, w, c))
        dyd = dy.to(DEV).contiguous()
        assert lib.frcnn_maxpool3x3s2_bwd(xd.data_ptr(), dyd.data_ptr(), out.data_ptr(), n, h, w, c, stream) == 0
    bands_intact("maxpool3x3s2", buf, out)
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", POOL3_CASES, ids=lambda c: "%dx%d-%s" % (c[0] + (c[1],)))
def test_maxpool3x3_carries_the_poison(hip, case):
    x, xp, dy, R, Rb, idx = pool3_case(*case)
    P = pool3_device(xp)
    judge("maxpool3x3s2_fwd %s" % (case,), P, pool3_device(x), R)
    assert torch.equal(_bits(P)[~torch.isnan(R)], _bits(R)[~torch.isnan(R)])          # a selection: bit for bit
    # backward: every window's dy lands on torch's winner.  A pixel adds at most four dy: 1e-6 against autograd, the bar of
    # test_maxpool_bwd_edges; the channels without poison keep their bits, and per channel sum(dx) == sum(dy)
    Pb, Cb = pool3_device(xp, dy), pool3_device(x, dy)
    assert bool(torch.isfinite(Pb).all())
    bar = 1e-6 * max(1.0, float(Rb.abs().max()))
    assert float((Pb - Rb).abs().max()) <= bar, "maxpool3x3s2_bwd %s: off autograd by %.3e" % (case, float((Pb - Rb).abs().max()))
    nan_pixels = torch.isnan(xp)
    assert torch.equal(Pb[nan_pixels] != 0, Rb[nan_pixels] != 0) and bool((Pb[nan_pixels] != 0).any() or case[1] == "inf_alone")
    others = [c for c in range(POOL_C) if c != POOL_CH]
    assert torch.equal(_bits(Pb[..., others]), _bits(Cb[..., others]))
    conservation = 3 * (U / 2) * dy.double().abs().sum((0, 1, 2)) + 1e-30
    assert bool(((Pb.double().sum((0, 1, 2)) - dy.double().sum((0, 1, 2))).abs() <= conservation).all())


POOL2_CASES = ["nan_alone", "nan_next_to_inf", "two_nans", "inf_alone"]


@functools.lru_cache(maxsize=None)
def pool2_case(pattern):
    """z -> relu -> max_pool2d(2, 2) on a 5 x 7 map (a trailing row and column in no window); autograd in float32."""
    g = torch.Generator().manual_seed(950)
    z = torch.randn((2, 5, 7, POOL_C), generator=g)
    zp = z.clone()
    zp[1, 2, 4, POOL_CH] = INF if pattern == "inf_alone" else NAN
    if pattern == "nan_next_to_inf":
        zp[1, 2, 5, POOL_CH] = INF
    if pattern == "two_nans":
        zp[1, 3, 5, POOL_CH] = NAN
    zr = zp.permute(0, 3, 1, 2).clone().requires_grad_(True)
    a = F.relu(zr)
    a.retain_grad()
    y = F.max_pool2d(a, 2, 2)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return F.relu(z), nhwc(a), nhwc(dy), nhwc(y), nhwc(a.grad), nhwc(zr.grad)


@pytest.mark.parametrize("pattern", POOL2_CASES)
def test_cpu_reference_maxpool2x2(pattern):
    a0, a, dy, R, Rb, Rz = pool2_case(pattern)
    assert host_check(pattern, R)
    if pattern != "inf_alone":
        assert bool(torch.isnan(R).any()) and not bool(torch.isinf(R).any())
        # relu's backward passes the gradient of a NaN activation: the relu_mask form must hand the window's dy to the NaN
        assert bool(torch.isfinite(Rz).all()) and bool((Rz[torch.isnan(a)] != 0).any()) and torch.equal(Rz[torch.isnan(a)], Rb[torch.isnan(a)])


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", POOL2_CASES)
def test_maxpool2x2_carries_the_poison(hip, pattern):
    ops = _ops()
    a0, a, dy, R, Rb, Rz = pool2_case(pattern)

    def fwd(x):
        buf, out = out_view(tuple(R.shape))
        ops.maxpool2x2s2_nhwc(x.to(DEV), out=out)
        bands_intact("maxpool2x2s2", buf, out)
        return out.cpu()

    def bwd(x, relu):
        buf, out = out_view(tuple(x.shape))
        ops.maxpool2x2s2_bwd(x.to(DEV), dy.to(DEV), relu=relu, out=out)
        bands_intact("maxpool2x2s2_bwd", buf, out)
        return out.cpu()

    judge("maxpool2x2s2_fwd %s" % pattern, fwd(a), fwd(a0), R)
    for relu, want in ((False, Rb), (True, Rz)):                     # a routing: equal to autograd, no tolerance
        P = bwd(a, relu)
        assert bool((P == want).all()), "maxpool2x2s2_bwd relu=%s %s: differs from autograd at %s" % (
            relu, pattern, (P != want).nonzero()[0].tolist())
        others = [c for c in range(POOL_C) if c != POOL_CH]
        assert torch.equal(_bits(P[..., others]), _bits(bwd(a0, relu)[..., others]))


# ================================================================================================
# 5. train-mode BatchNorm
# ================================================================================================
BN_SHAPE = (257, 132)
BN_CHANNEL = 70
BN_CASES = [(mode, kind) for mode in ("relu", "relu_res") for kind in ("nan", "+inf")]


def bn_float64(inp):
    y = inp["y"].double()
    o = F.batch_norm(y, None, None, inp["gamma"].double(), inp["beta"].double(), True, 0.1, BN.EPS)
    if inp["res"] is not None:
        o = o + inp["res"].double()
    return torch.relu(o) if inp["relu"] else o


def bn_inputs(mode, kind):
    inp, _ = BN.bn_case(BN_SHAPE[0], BN_SHAPE[1], mode)
    return inp, dict(inp, y=poison(inp["y"], (101, BN_CHANNEL), kind))


@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "%s-%s" % c)
def test_cpu_reference_batchnorm(case):
    inp, dirty = bn_inputs(*case)
    R, R0 = bn_float64(dirty), bn_float64(inp)
    others = torch.arange(BN_SHAPE[1]) != BN_CHANNEL
    assert bool(torch.isnan(R[:, BN_CHANNEL]).all()), "torch: one non-finite input makes the whole channel NaN behind the ReLU"
    assert torch.equal(R[:, others], R0[:, others]) and bool(torch.isfinite(R0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "%s-%s" % c)
def test_batchnorm_carries_the_poison(hip, case):
    ops = _ops()
    inp, dirty = bn_inputs(*case)
    C, P = BN._cpu(BN.run_device(ops, inp)), BN._cpu(BN.run_device(ops, dirty))
    assert bool(torch.isnan(P["out"][:, BN_CHANNEL]).all()), "out[:, %d] must be all NaN" % BN_CHANNEL
    others = torch.arange(BN_SHAPE[1]) != BN_CHANNEL
    for name in BN.OUTPUTS:
        if C[name] is not None:
            assert torch.equal(_bits(P[name][..., others]), _bits(C[name][..., others])), name
    assert bool(torch.isfinite(C["out"]).all())


def bn_mask_case(mode="relu_res"):
    """A NaN in the stored output of a channel, at a row where the ReLU had closed the mask."""
    inp, _ = BN.bn_case(BN_SHAPE[0], BN_SHAPE[1], mode)
    out = bn_float64(inp).float()
    rows = (out[:, 9] == 0).nonzero().reshape(-1)
    return inp, out, (int(rows[len(rows) // 2]), 9)


@pytest.mark.parametrize("mode", ["relu", "relu_res"])
def test_cpu_reference_batchnorm_backward_mask(mode):
    inp, out, at = bn_mask_case(mode)
    x = out.clone()
    x[at] = NAN
    x.requires_grad_(True)
    F.relu(x).backward(inp["dout"])                                  # relu(out) == out where out > 0: the mask of the fused ReLU
    assert float(x.grad[at]) == float(inp["dout"][at]) != 0.0 and float(out[at]) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["relu", "relu_res"])
def test_batchnorm_backward_mask_opens_for_a_nan_output(hip, mode):
    """bn_train_bwd with a NaN in ``out``, with relu and with relu plus residual: d_res there is dout (torch: out <= 0 ? 0 :
    dout); d_beta = sum g and d_gamma = sum g * xhat of the channel take it in (the column sums of bn_partial_kernel<BWD>, against
    float64 sums over torch's mask with the device's own saved statistics; one rounding of the float64 sum to fp32: U / 2 of
    |sum| <= sum |terms|, taken as U); every other channel keeps its bits."""
    ops = _ops()
    inp, _, at = bn_mask_case(mode)
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    y, gamma, dout = dev(inp["y"]), dev(inp["gamma"]), dev(inp["dout"])
    out, mean, invstd = ops.bn_train_fwd(y, gamma, dev(inp["beta"]), BN.EPS, BN.MOM, dev(inp["rm"]), dev(inp["rv"]), dev(inp["res"]), True)
    assert float(out[at]) == 0.0
    dirty = out.clone()
    dirty[at] = NAN
    clean = [t.cpu() for t in ops.bn_train_bwd(dout, out, y, gamma, mean, invstd, relu=True, want_res=True)]
    got = [t.cpu() for t in ops.bn_train_bwd(dout, dirty, y, gamma, mean, invstd, relu=True, want_res=True)]
    want = torch.where(dirty.cpu() <= 0, torch.zeros_like(inp["dout"]), inp["dout"])
    assert torch.equal(got[1], want), "d_res is dout behind torch's mask"
    assert float(got[1][at]) == float(inp["dout"][at]) and float(clean[1][at]) == 0.0
    others = torch.arange(BN_SHAPE[1]) != at[1]
    for a, b in zip(got, clean):
        assert torch.equal(_bits(a[..., others]), _bits(b[..., others]))
    col = want[:, at[1]].double()
    assert abs(float(got[3][at[1]]) - float(col.sum())) <= BN_SHAPE[0] * U * float(col.abs().sum())
    assert float(got[3][at[1]]) != float(clean[3][at[1]])
    xhat = (inp["y"][:, at[1]].double() - float(mean[at[1]])) * float(invstd[at[1]])
    terms = col * xhat
    print("d_gamma: device %.9g, float64 %.9g, bar %.3g" % (float(got[2][at[1]]), float(terms.sum()), U * float(terms.abs().sum())))
    assert abs(float(got[2][at[1]]) - float(terms.sum())) <= U * float(terms.abs().sum())
    assert float(got[2][at[1]]) != float(clean[2][at[1]])


# ================================================================================================
# 6. depthwise 3x3, the ReLU6 clamp and the activation backward kernels
# ================================================================================================
DW_SHAPE = (2, 5, 7, 8)                                              # W = 7: a ragged strip of FRCNN_DWCONV_STRIP outputs
DW_CASES = ([(stride, 6.0, operand, "nan") for stride in (1, 2) for operand in ("x", "w", "scale", "shift")] +
            [(1, INF, "x", "+inf"), (1, INF, "x", "-inf"), (2, INF, "shift", "+inf")])


@functools.lru_cache(maxsize=None)
def dw_operands():
    n, h, w, c = DW_SHAPE
    gen = torch.Generator().manual_seed(7100)
    nz = lambda t: torch.where(t == 0, torch.ones_like(t), t)
    return {"x": nz(torch.randint(-3, 4, DW_SHAPE, generator=gen).double()), "w": nz(torch.randint(-3, 4, (3, 3, c), generator=gen).double()),
            "scale": torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (c,), generator=gen)],
            "shift": torch.randint(-3, 4, (c,), generator=gen).double()}


def dw_float64(t, stride, cap):
    """min(relu(conv * scale + shift), cap) as nn.ReLU6 / nn.ReLU evaluate it (integers: exact in fp32, in any order)."""
    c = t["x"].shape[-1]
    y = F.conv2d(t["x"].permute(0, 3, 1, 2), t["w"].permute(2, 0, 1)[:, None], stride=stride, padding=1, groups=c).permute(0, 2, 3, 1)
    return torch.clamp(torch.relu(y * t["scale"] + t["shift"]), max=cap).contiguous()


@functools.lru_cache(maxsize=None)
def dw_reference(case):
    stride, cap, operand, kind = case
    t = dict(dw_operands())
    index = {"x": (1, 2, 3, 5), "w": (1, 1, 5), "scale": (5,), "shift": (5,)}[operand]
    t[operand] = poison(t[operand], index, kind)
    return t, dw_float64(t, stride, cap)


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "s%d-cap%s-%s-%s" % c)
def test_cpu_reference_depthwise(case):
    _, R = dw_reference(case)
    assert host_check(str(case), R) and bool(torch.isfinite(dw_float64(dw_operands(), case[0], case[1])).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "s%d-cap%s-%s-%s" % c)
def test_depthwise_carries_the_poison(hip, case):
    ops = _ops()
    stride, cap, operand, kind = case
    t, R = dw_reference(case)

    def run(t):
        d = {k: v.float().to(DEV).contiguous() for k, v in t.items()}
        buf, out = out_view(tuple(R.shape))
        ops.depthwise_conv3x3_nhwc(d["x"], d["w"], d["scale"], d["shift"], stride=stride, relu=True, out_cap=cap, out=out)
        bands_intact("dwconv", buf, out)
        return out.cpu()

    C = run(dw_operands())
    assert torch.equal(C.double(), dw_float64(dw_operands(), stride, cap))
    judge(str(case), run(t), C, R, values=True, R0=dw_float64(dw_operands(), stride, cap))


@functools.lru_cache(maxsize=None)
def act_case():
    """A ReLU6 output y (23 rows x 12 channels: 276 = 4 * 69 floats; its 1-D form of 275 has a tail of 3), dy, scale."""
    gen = torch.Generator().manual_seed(7200)
    y = torch.clamp(torch.relu(torch.randn((23, 12), generator=gen) * 4), max=6.0)
    return y, torch.randn((23, 12), generator=gen), torch.rand(12, generator=gen) + 0.5


def act_bwd_float32(dy, y, scale, cap):
    """hardtanh_backward / threshold_backward: (y <= 0 || y >= cap) ? 0 : dy, then the folded scale."""
    g = torch.where((y <= 0) | (y >= cap), torch.zeros_like(dy), dy)
    return g, g * scale


def test_cpu_reference_activation_kernels():
    y, dy, scale = act_case()
    assert bool((y == 0).any()) and bool((y == 6).any()) and bool(((y > 0) & (y < 6)).any())
    yr = y.clone().requires_grad_(True)
    F.hardtanh(yr, 0.0, 6.0).backward(dy)                            # relu6 of a relu6 output: the mask the kernels rebuild from y
    assert torch.equal(yr.grad, act_bwd_float32(dy, y, scale, 6.0)[0])
    # a NaN activation: torch's element-wise rule (and its device kernel) is (y <= 0 || y >= cap) ? 0 : g, which is open.  Asked
    # of ONE element, because the host's vectorised hardtanh_backward loop (tensors of a vector width and more) answers 0 for a NaN
    # where its own scalar loop answers g (torch 2.10); threshold_backward (relu) is open in both, asked of the whole tensor here
    yn = torch.tensor([NAN], requires_grad=True)
    F.hardtanh(yn, 0.0, 6.0).backward(dy[11, 5:6])
    assert float(yn.grad) == float(dy[11, 5]) == float(act_bwd_float32(dy[11, 5:6], yn.detach(), 1.0, 6.0)[0])
    yn = poison(y, (11, 5), "nan").requires_grad_(True)
    F.relu(yn).backward(dy)
    assert torch.equal(yn.grad, act_bwd_float32(dy, yn.detach(), scale, INF)[0]) and float(yn.grad[11, 5]) == float(dy[11, 5])


@pytest.mark.gpu
def test_clamp_max_keeps_nan(hip):
    ops = _ops()
    y = act_case()[0].reshape(-1)[:275] * 2 - 3                      # values on both sides of the cap
    for at in (6, 274):                                              # the float4 body and the 3-element tail
        for kind in KINDS:
            x = poison(y, (at,), kind)
            buf, view = guarded(275, fill=SENTINEL, guard=BAND)
            view.copy_(x)
            ops.clamp_max_(view, 6.0)
            assert bool(guards_flag(buf, 275, BAND))
            got, want = view.cpu(), torch.clamp(x, max=6.0)
            assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(want).any() == (kind == "nan"))
            assert torch.equal(_bits(got)[~torch.isnan(want)], _bits(want)[~torch.isnan(want)])


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["act_bwd_cap", "act_bwd"])
@pytest.mark.parametrize("operand,kind", [("y", "nan"), ("dy", "nan"), ("dy", "+inf")])
def test_activation_backward_follows_torch(hip, entry, operand, kind):
    """y NaN at a closed mask element (y == 0): it opens.  dy NaN / Inf at an open one: it passes; at a closed one it is 0."""
    ops = _ops()
    y, dy, scale = act_case()
    cap = 6.0 if entry == "act_bwd_cap" else INF
    closed, opened = (y == 0).nonzero()[3], ((y > 0) & (y < 6)).nonzero()[3]
    yp, dyp = y, dy
    if operand == "y":
        yp = poison(y, tuple(closed.tolist()), kind)
    else:
        dyp = poison(poison(dy, tuple(opened.tolist()), kind), tuple(closed.tolist()), kind)

    def run(dy, y):
        if entry == "act_bwd_cap":
            buf, out = out_view(tuple(dy.shape))
            ops.act_bwd_cap(dy.to(DEV), y.to(DEV), scale.to(DEV), relu=True, cap=cap, out=out)
            bands_intact(entry, buf, out)
            return None, out.cpu()
        d_conv, d_res = ops.act_bwd(dy.to(DEV), y.to(DEV), scale.to(DEV), relu=True, want_res=True)
        return d_res.cpu(), d_conv.cpu()

    (res_c, conv_c), (res_p, conv_p) = run(dy, y), run(dyp, yp)
    want_res, want_conv = act_bwd_float32(dyp, yp, scale, cap)
    touched = (want_conv != act_bwd_float32(dy, y, scale, cap)[1]) | torch.isnan(want_conv)
    assert int(touched.sum()) == 1
    if operand == "y":
        assert float(want_conv[tuple(closed.tolist())]) != 0.0 and bool(torch.isfinite(want_conv).all())
        assert torch.equal(_bits(conv_p)[touched], _bits(want_conv)[touched])
        assert torch.equal(_bits(conv_p)[~touched], _bits(conv_c)[~touched])
    else:
        judge("%s d_conv" % entry, conv_p, conv_c, want_conv, R0=act_bwd_float32(dy, y, scale, cap)[1])
    if res_p is not None:
        assert torch.equal(torch.isnan(res_p), torch.isnan(want_res))
        assert torch.equal(_bits(res_p)[~torch.isnan(want_res)], _bits(want_res)[~torch.isnan(want_res)])


# ================================================================================================
# 7. plain-arithmetic kernels: a guard against future shortcuts
# ================================================================================================
# A whole channel (or one logit / delta) is poisoned: every output that reads it is NaN, everything else keeps its bits.
PLAIN_CH = 5


def _channel_verdict(label, P, C, R):
    """Last axis = channels: rule 1 against R, and every channel but PLAIN_CH bit-equal to the clean run."""
    P, C = P.detach().cpu(), C.detach().cpu()
    judge(label, P, C, R, "superset")
    others = [c for c in range(P.shape[-1]) if c != PLAIN_CH]
    assert torch.equal(_bits(P[..., others]), _bits(C[..., others])), "%s: another channel changed" % label


@functools.lru_cache(maxsize=None)
def plain_case():
    gen = torch.Generator().manual_seed(7300)
    x = torch.randn((3, 7, 7, 16), generator=gen)
    small, lateral = torch.randn((2, 3, 4, 8), generator=gen), torch.randn((2, 7, 9, 8), generator=gen)
    feat = torch.randn((1, 9, 11, 16), generator=gen)
    scale, shift = torch.rand(16, generator=gen) + 0.5, torch.randn(16, generator=gen)
    from test_roi_align_kernels import _CH_ROIS
    rois = torch.tensor(_CH_ROIS, dtype=torch.float32)
    nanch = lambda t: poison(t, (Ellipsis, PLAIN_CH), "nan")
    from oracle import frcnn_oracle as O

    def roi_ref(f):
        pooled = O.roi_align(f.permute(0, 3, 1, 2).contiguous(), rois, 7, 1.0, 0).permute(0, 2, 3, 1)
        return torch.relu(pooled * scale + shift)
    up = lambda s: F.interpolate(s.permute(0, 3, 1, 2), size=lateral.shape[1:3], mode="bilinear", align_corners=False).permute(0, 2, 3, 1) + lateral
    return dict(x=x, xp=nanch(x), mean=nanch(x).permute(0, 3, 1, 2).mean(3).mean(2), small=small, smallp=nanch(small), lateral=lateral,
                up=up(nanch(small)), feat=feat, featp=nanch(feat), rois=rois, scale=scale, shift=shift, roi=roi_ref(nanch(feat)),
                roi_clean=roi_ref(feat))


def test_cpu_reference_plain_arithmetic():
    d = plain_case()
    assert bool(torch.isnan(d["mean"][:, PLAIN_CH]).all()) and host_check("spatial_mean", d["mean"])
    assert bool(torch.isnan(d["up"][..., PLAIN_CH]).all()) and host_check("upsample", d["up"])
    # RoIAlign + folded BatchNorm + ReLU: a RoI that samples the map has its poisoned channel NaN behind the ReLU
    sampled = (d["roi_clean"] != torch.relu(d["shift"])).flatten(1).any(1)
    assert bool(sampled.any()) and bool(torch.isnan(d["roi"][sampled][..., PLAIN_CH]).flatten(1).any(1).all())
    assert host_check("roi_align", d["roi"]) and bool(torch.isfinite(d["roi_clean"]).all())


@pytest.mark.gpu
def test_spatial_mean_and_upsample_carry_a_nan_channel(hip):
    ops, d = _ops(), plain_case()
    dev = lambda k: d[k].to(DEV).contiguous()
    _channel_verdict("spatial_mean", ops.spatial_mean(dev("xp")), ops.spatial_mean(dev("x")), d["mean"])
    _channel_verdict("upsample_bilinear_add", ops.upsample_bilinear_add(dev("smallp"), dev("lateral")),
                     ops.upsample_bilinear_add(dev("small"), dev("lateral")), d["up"])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 3], ids=["per_sample", "planned"])       # (the map-resident kernel has no epilogue)
def test_roi_align_with_relu_epilogue_carries_a_nan_channel(hip, variant):
    ops, d = _ops(), plain_case()
    dev = lambda k: d[k].to(DEV).contiguous()

    def run(feat):
        buf, out = out_view(tuple(d["roi"].shape))
        hip.frcnn_roi_align_set_variant(variant)
        try:
            ops.roi_align_nhwc(dev(feat), dev("rois"), 7, 1.0, 0, out=out, scale=dev("scale"), shift=dev("shift"), relu=True)
            torch.cuda.synchronize()
        finally:
            hip.frcnn_roi_align_set_variant(0)
        bands_intact("roi_align", buf, out)
        return out.cpu()

    _channel_verdict("roi_align variant %d" % variant, run("featp"), run("feat"), d["roi"])


@functools.lru_cache(maxsize=None)
def head_case(k):
    gen = torch.Generator().manual_seed(7400 + k)
    r, p, c = 6, 2, 64
    x = torch.randn((r, p, p, c), generator=gen)
    w_cls, b_cls = torch.randn((k, c), generator=gen) * 0.1, torch.randn(k, generator=gen) * 0.1
    w_box, b_box = torch.randn((4 * k, c), generator=gen) * 0.1, torch.randn(4 * k, generator=gen) * 0.1
    rois = torch.tensor([[0, 10.0 + i, 12.0, 60.0 + 3 * i, 50.0] for i in range(r)])
    xp = poison(x, (2, 1, 0, 7), "nan")                                # one feature of RoI 2
    fc7 = xp.double().permute(0, 3, 1, 2).mean(3).mean(2)
    prob = F.softmax(F.linear(fc7, w_cls.double(), b_cls.double()), 1)
    return dict(x=x, xp=xp, w_cls=w_cls, b_cls=b_cls, w_box=w_box, b_box=b_box, rois=rois, prob=prob)


@pytest.mark.parametrize("k", [3, 21], ids=["narrow", "wide"])
def test_cpu_reference_head(k):
    prob = head_case(k)["prob"]
    assert bool(torch.isnan(prob[2]).all()) and bool(torch.isfinite(prob[[0, 1, 3, 4, 5]]).all())   # F.softmax: the row is NaN


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 21], ids=["narrow", "wide"])
def test_head_softmax_carries_a_nan_logit(hip, k):
    ops, d = _ops(), head_case(k)
    dev = lambda key: d[key].to(DEV).contiguous()
    assert ops.head_uses_wide_form(k, 4) == (k == 21)

    def run(x):
        heads = [dev(n) for n in ("w_cls", "b_cls", "w_box", "b_box", "rois")] + [[0.1, 0.1, 0.2, 0.2], [0.0] * 4, 1.0]
        if k == 21:
            return ops.head_softmax_decode_wide(ops.spatial_mean(dev(x)), *heads)
        return ops.head_fc_softmax_decode(dev(x), *heads)

    C, P = run("x"), run("xp")
    judge("cls_prob K=%d" % k, P["cls_prob"], C["cls_prob"], d["prob"], "superset")
    rest = [0, 1, 3, 4, 5]
    for name in ("cls_score", "cls_prob", "bbox_pred", "pred_boxes"):
        assert bool(torch.isnan(P[name][2]).all()), name
        assert torch.equal(_bits(P[name].cpu()[rest]), _bits(C[name].cpu()[rest])), name


@pytest.mark.gpu
def test_losses_carry_a_nan_logit_or_delta(hip):
    """rpn_loss and det_loss on cases of tests/test_loss_stat_kernels.py: a NaN logit of a labelled anchor / RoI makes the
    cross entropy NaN, a NaN delta under a non-zero inside weight the box loss - as F.cross_entropy and the smooth-L1 sum do."""
    import test_loss_stat_kernels as L
    ops = _ops()
    inp, ref, _, count = L.rpn_case((204, 25, 152), "normal")
    a = inp["a"]
    labels = inp["labels"].view(204, a)
    at = (labels >= 0).nonzero()[7]
    fg = (inp["inside"].view(204, a, 4)[..., 0] > 0).nonzero()[7]
    assert count > 0 and bool(torch.isfinite(ref["ce"])) and bool(torch.isfinite(ref["box"]))
    args = lambda rpn: [rpn.to(DEV), a] + [inp[k].to(DEV) for k in ("labels", "targets", "inside", "outside")]
    clean = ops.rpn_loss(*args(inp["rpn"]))[0].cpu()
    assert bool(torch.isfinite(clean).all())
    logit = ops.rpn_loss(*args(poison(inp["rpn"], (int(at[0]), int(at[1])), "nan")))[0].cpu()
    assert torch.isnan(logit[0]) and float(logit[1]) == float(clean[1]) and float(logit[2]) == float(clean[2])
    delta = ops.rpn_loss(*args(poison(inp["rpn"], (int(fg[0]), 2 * a + 4 * int(fg[1]) + 1), "nan")))[0].cpu()
    assert torch.isnan(delta[1]) and float(delta[0]) == float(clean[0])
    inp, ref, _ = L.det_case(257, 4, "plain4", "normal")
    row = int((inp["iw"].sum(1) > 0).nonzero()[3])
    col = int((inp["iw"][row] > 0).nonzero()[0])
    dargs = lambda cls, bp: [t.to(DEV) for t in (cls, inp["lab"], bp, inp["bt"], inp["iw"], inp["ow"])]
    clean = ops.det_loss(*dargs(inp["cls"], inp["bp"]))[0].cpu()
    assert bool(torch.isfinite(clean).all())
    logit = ops.det_loss(*dargs(poison(inp["cls"], (row, 1), "nan"), inp["bp"]))[0].cpu()
    assert torch.isnan(logit[0]) and float(logit[1]) == float(clean[1])
    delta = ops.det_loss(*dargs(inp["cls"], poison(inp["bp"], (row, col), "nan")))[0].cpu()
    assert torch.isnan(delta[1]) and float(delta[0]) == float(clean[0])


# ================================================================================================
# 8. the scalar tail of act_bwd_cap and the input cap of the depthwise kernels
# ================================================================================================
@pytest.mark.gpu
def test_act_bwd_cap_scalar_tail_follows_torch(hip):
    """5 x 3 = 15 floats: three float4 and a tail of three, which act_bwd_cap_kernel masks one by one.  In the tail: a NaN y on a
    closed element opens it, a NaN dy passes an open element and is 0 behind a closed one."""
    ops = _ops()
    y = torch.tensor([[0.0, 2.0, 6.0], [1.0, 0.0, 3.0], [6.0, 5.0, 0.0], [2.0, 0.0, 1.0], [0.0, 3.0, 0.0]])
    dy = torch.arange(1.0, 16.0).view(5, 3) / 4
    scale = torch.tensor([0.5, 2.0, 1.5])
    yp, dyp = poison(y, (4, 0), "nan"), poison(poison(dy, (4, 1), "nan"), (4, 2), "nan")

    def run(dy, y):
        buf, out = out_view((5, 3))
        ops.act_bwd_cap(dy.to(DEV), y.to(DEV), scale.to(DEV), relu=True, cap=6.0, out=out)
        bands_intact("act_bwd_cap", buf, out)
        return out.cpu()

    want = act_bwd_float32(dyp, yp, scale, 6.0)[1]
    assert want[4].tolist()[0] == float(dy[4, 0] * scale[0]) and torch.isnan(want[4, 1]) and float(want[4, 2]) == 0.0
    got, clean = run(dyp, yp), run(dy, y)
    assert torch.equal(_bits(clean), _bits(act_bwd_float32(dy, y, scale, 6.0)[1])) and float(clean[4, 0]) == 0.0
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(_bits(got)[~torch.isnan(want)], _bits(want)[~torch.isnan(want)])


@functools.lru_cache(maxsize=None)
def dw_in_cap_case():
    """min(x, 6) in front of the depthwise convolution (the ReLU6 cap of the pointwise layer before it, folded into the load):
    integers, some above the cap, and one NaN - torch.clamp hands it through."""
    t = dict(dw_operands())
    x = t["x"].clone()
    x[0, 1, 1, 2] = x[1, 3, 5, 6] = 9.0                              # above the cap
    xp = poison(x, (1, 2, 3, PLAIN_CH), "nan")
    gen = torch.Generator().manual_seed(7500)
    dy = torch.randint(1, 4, DW_SHAPE, generator=gen).double()

    def ref(x):
        w = t["w"].permute(2, 0, 1)[:, None].clone().requires_grad_(True)
        y = F.conv2d(torch.clamp(x, max=6.0).permute(0, 3, 1, 2), w, padding=1, groups=DW_SHAPE[3])
        y.backward(dy.permute(0, 3, 1, 2))
        return y.detach().permute(0, 2, 3, 1).contiguous(), w.grad.detach()
    return t, x, xp, dy, ref(x), ref(xp)


def test_cpu_reference_depthwise_input_cap():
    _, x, xp, dy, (y0, dw0), (y, dw) = dw_in_cap_case()
    assert host_check("dwconv in_cap forward", y) and bool(torch.isfinite(y0).all()) and bool(torch.isfinite(dw0).all())
    assert bool(torch.isnan(dw[PLAIN_CH]).all()) and bool(torch.isfinite(dw[[c for c in range(8) if c != PLAIN_CH]]).all())
    assert not torch.equal(y0, F.conv2d(x.permute(0, 3, 1, 2), dw_operands()["w"].permute(2, 0, 1)[:, None], padding=1, groups=8).permute(0, 2, 3, 1))


@pytest.mark.gpu
def test_depthwise_input_cap_keeps_nan(hip):
    """depthwise_conv3x3_nhwc and depthwise_conv3x3_bwd_weight with in_cap = 6 and a NaN in x: the forward's 3 x 3 neighbourhood
    of that channel and every tap of its filter gradient are NaN, everything else keeps its bits."""
    ops = _ops()
    t, x, xp, dy, (y0, dw0), (y, dw) = dw_in_cap_case()
    dev = lambda v: v.float().to(DEV).contiguous()

    def fwd(x):
        buf, out = out_view(DW_SHAPE)
        ops.depthwise_conv3x3_nhwc(dev(x), dev(t["w"]), in_cap=6.0, out=out)
        bands_intact("dwconv in_cap", buf, out)
        return out.cpu()

    def wgrad(x):
        buf, out = out_view((DW_SHAPE[3], 1, 3, 3))
        ops.depthwise_conv3x3_bwd_weight(dev(x), dev(dy), None, in_cap=6.0, out=out)
        bands_intact("dwconv bwd_weight in_cap", buf, out)
        return out.cpu()

    C = fwd(x)
    assert torch.equal(C.double(), y0)
    judge("dwconv in_cap forward", fwd(xp), C, y, values=True)
    Cw = wgrad(x)
    assert torch.equal(Cw.double(), dw0)
    channel = torch.zeros(dw.shape, dtype=torch.bool)
    channel[PLAIN_CH] = True
    judge("dwconv in_cap filter gradient", wgrad(xp), Cw, dw, footprint=channel, values=True)
