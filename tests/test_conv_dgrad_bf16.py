"""The bf16-operand data gradient (frcnn_conv2d_bwd_data_bf16) through ``ops``, against float64 on the host.

    dx = act_bwd(conv_transpose(bf16(dy), bf16(w)) [+ add])          fp32 accumulation, act_bwd = mask by act_y > 0, times act_scale

The shapes of tests/test_conv_wgrad_bf16.py without the strided 1x1, whose data gradient stays fp32 (the entry point refuses
it).  The filter operand is conv2d_pack_bf16(conv2d_transpose_filter(w)).
  * integer operands in [-3, 3]: equal to float64 bit for bit, with ``add``, the mask and a power-of-two scale too;
  * normal operands against float64 on the bf16-ROUNDED operands: within n * 2^-24 * sum|products|, n = K*R*S accumulated terms;
  * normal operands against float64 on the UNROUNDED operands: within 2^-7 * sum|products|, and not equal to it;
  * ``add`` / ``act_y`` / ``act_scale`` on normal operands: bit-equal to the same three fp32 operations applied on the host to the
    plain result (one addition, one select, one multiplication per element: nothing to reorder);
  * two runs are bit-equal; NaN guard bands around dx and the workspace are intact and every element of dx is written.
"""
import pytest

import test_conv_wgrad_bf16 as W
from guarded_buffers import DEV, guarded, guards_intact

NAMES = [n for n in W.SHAPES if n != "batch_1x1s2"]
_CACHE = {}


def operands(name, kind):
    """(dy (n,ho,wo,k), w (k,r,s,c)) as float64 host tensors holding fp32 values."""
    import torch
    n, h, w, c, k, r, stride, pad = W.SHAPES[name]
    ho, wo = W.out_hw(h, w, r, stride, pad)
    gen = torch.Generator().manual_seed(sorted(W.SHAPES).index(name) * 11 + (3 if kind == "int" else 4))
    if kind == "int":
        return (torch.randint(-3, 4, (n, ho, wo, k), generator=gen).double(), torch.randint(-3, 4, (k, r, r, c), generator=gen).double())
    return (torch.randn((n, ho, wo, k), generator=gen, dtype=torch.float32).double(),
            torch.randn((k, r, r, c), generator=gen, dtype=torch.float32).double())


def dx_float64(name, dy, wt):
    """conv_transpose in float64: (n, h, w, c)."""
    import torch.nn.functional as F
    n, h, w, c, k, r, stride, pad = W.SHAPES[name]
    cols = dy.reshape(n, -1, k) @ wt.permute(0, 3, 1, 2).reshape(k, c * r * r)       # (n, L, (c, r, s))
    return F.fold(cols.transpose(1, 2), (h, w), (r, r), padding=pad, stride=stride).permute(0, 2, 3, 1).contiguous()


def reference(name, kind):
    if (name, kind) not in _CACHE:
        dy, wt = operands(name, kind)
        ref = {"dy": dy, "w": wt, "exact": dx_float64(name, dy, wt)}
        if kind != "int":
            ref["abs"] = dx_float64(name, dy.abs(), wt.abs())
            ref["rounded"] = dx_float64(name, W.rbf16(dy), W.rbf16(wt))
            ref["abs_rounded"] = dx_float64(name, W.rbf16(dy).abs(), W.rbf16(wt).abs())
        _CACHE[(name, kind)] = ref
    return _CACHE[(name, kind)]


def epilogue_operands(name, kind):
    """(add, act_y, act_scale) for the shape: integers / a power-of-two scale for the exact case."""
    import torch
    n, h, w, c, k, r, stride, pad = W.SHAPES[name]
    gen = torch.Generator().manual_seed(77)
    if kind == "int":
        add = torch.randint(-3, 4, (n, h, w, c), generator=gen).double()
        scale = 2.0 ** torch.randint(-2, 3, (c,), generator=gen).double()
    else:
        add = torch.randn((n, h, w, c), generator=gen, dtype=torch.float32).double()
        scale = torch.randn((c,), generator=gen, dtype=torch.float32).double()
    act_y = torch.randn((n, h, w, c), generator=gen, dtype=torch.float32).clamp_min(0).double()
    return add, act_y, scale


def run_device(name, dy, wt, add=None, act_y=None, act_scale=None):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    n, h, w, c, k, r, stride, pad = W.SHAPES[name]
    dev = lambda t: t.float().to(DEV) if t is not None else None
    w_t = ops.conv2d_transpose_filter(dev(wt))
    packed = ops.conv2d_pack_bf16(w_t)
    ws_bytes = int(_hip.load().frcnn_conv2d_bwd_data_bf16_ws_bytes(n, h, w, c, k, r, r, stride, pad))
    ws_floats = max((ws_bytes + 3) // 4, 4)
    wbuf, ws = guarded(ws_floats)
    obuf, out = guarded(n * h * w * c)
    res = ops.conv2d_bwd_data_bf16(dev(dy), packed, (n, h, w, c), stride=stride, pad=pad, add=dev(add), act_y=dev(act_y),
                                   act_scale=dev(act_scale), out=out.view(n, h, w, c), ws=ws)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert guards_intact(obuf, out.numel()), "%s: wrote outside dx" % name
    assert guards_intact(wbuf, ws_floats), "%s: wrote outside the workspace" % name
    host = out.cpu().double().view(n, h, w, c)
    assert not torch.isnan(host).any(), "%s: an element of dx was not written" % name
    return host


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_integer_operands_are_exact(hip, name):
    import torch
    ref = reference(name, "int")
    assert torch.equal(run_device(name, ref["dy"], ref["w"]), ref["exact"])
    add, act_y, scale = epilogue_operands(name, "int")
    want = torch.where(act_y > 0, ref["exact"] + add, torch.zeros_like(add)) * scale
    assert torch.equal(run_device(name, ref["dy"], ref["w"], add, act_y, scale), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_normal_operands_within_the_bounds(hip, name):
    import torch
    n, h, w, c, k, r, stride, pad = W.SHAPES[name]
    terms = k * r * r
    ref = reference(name, "normal")
    got = run_device(name, ref["dy"], ref["w"])
    assert torch.equal(got, run_device(name, ref["dy"], ref["w"])), "two runs differ"
    err_r, bound_r = (got - ref["rounded"]).abs(), terms * 2.0 ** -24 * ref["abs_rounded"]
    err_u, bound_u = (got - ref["exact"]).abs(), 2.0 ** -7 * ref["abs"]
    print("%s: max err/bound against rounded operands %.3g, against unrounded operands %.3g"
          % (name, float((err_r / bound_r.clamp_min(1e-300)).max()), float((err_u / bound_u.clamp_min(1e-300)).max())))
    assert bool((err_r <= bound_r).all())
    assert bool((err_u <= bound_u).all())
    assert not torch.equal(got, ref["exact"].float().double()), "no rounding of the operands visible"


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_add_mask_and_scale_are_the_fp32_operations(hip, name):
    import torch
    ref = reference(name, "normal")
    plain = run_device(name, ref["dy"], ref["w"]).float()
    add, act_y, scale = epilogue_operands(name, "normal")
    summed = plain + add.float()
    assert torch.equal(run_device(name, ref["dy"], ref["w"], add=add).float(), summed)
    masked = torch.where(act_y > 0, summed, torch.zeros_like(summed))
    assert torch.equal(run_device(name, ref["dy"], ref["w"], add=add, act_y=act_y).float(), masked)
    assert torch.equal(run_device(name, ref["dy"], ref["w"], add=add, act_y=act_y, act_scale=scale).float(), masked * scale.float())


@pytest.mark.gpu
def test_strided_1x1_is_refused(hip):
    """The strided 1x1 data gradient writes a scattered output: it has no bf16 form, the wrapper and the library say so."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    n, h, w, c, k, r, stride, pad = W.SHAPES["batch_1x1s2"]
    dy = torch.zeros((n, 2, 2, k), dtype=torch.float32, device=DEV)
    packed = ops.conv2d_pack_bf16(torch.zeros((c, 1, 1, k), dtype=torch.float32, device=DEV))
    with pytest.raises(_hip.HipError):
        ops.conv2d_bwd_data_bf16(dy, packed, (n, h, w, c), stride=stride, pad=pad)
    dx = torch.full((n, h, w, c), float("nan"), dtype=torch.float32, device=DEV)
    rc = _hip.load().frcnn_conv2d_bwd_data_bf16(dy.data_ptr(), packed.data_ptr(), None, None, None, dx.data_ptr(), n, h, w, c, k,
                                                1, 1, stride, pad, None, 0, None)
    torch.cuda.synchronize()
    assert rc != 0 and bool(torch.isnan(dx).all())
