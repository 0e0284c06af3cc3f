"""Tensor-level wrappers over the C ABI (include/frcnn_hip.h).

torch is used here only as the owner of device memory and of the HIP stream; every computation is a
libfrcnn_hip.so kernel launched on ``torch.cuda.current_stream()``.  Nothing synchronises with the host,
so a sequence of these calls can be captured into one hipGraph.  CPU tensors are rejected: there is no
non-HIP execution path in this package.

Layouts: activations NHWC ``(N, H, W, C)`` contiguous fp32, filters KRSC ``(K, R, S, C)`` contiguous fp32.
"""
import ctypes

import os

import numpy as np
import torch

from . import _hip

# Shape log for bench.py / tuning: when PROFILE is a list, every conv2d_nhwc call appends its shape dict, in call order -
# the order of the call numbers conv_profile_end() reports with the per-dispatch durations.
PROFILE = None
# FLOP accounting for bench.py's training / LiDAR rooflines: when FLOPS is a dict, every forward / data-gradient /
# filter-gradient convolution call adds its direct-form FLOPs under 'fwd' / 'dgrad' / 'wgrad' and what the matrix pipe
# executes under '<kind>_executed' (a Winograd F(2x2,3x3) plan multiplies 16 values per 2x2 output tile instead of 36).
FLOPS = None


def flops_begin():
    global FLOPS
    FLOPS = {k: 0.0 for k in ('fwd', 'dgrad', 'wgrad', 'fwd_executed', 'dgrad_executed', 'wgrad_executed')}


def flops_end():
    global FLOPS
    out, FLOPS = FLOPS, None
    return out


def _log_flops(kind, direct, winograd=False):
    if FLOPS is not None:
        FLOPS[kind] += direct
        FLOPS[kind + '_executed'] += direct * (16.0 / 36.0 if winograd else 1.0)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _hip.HipError("%s must be a tensor on the MI355X (got %s); this package has no CPU path"
                            % (name, getattr(t, "device", type(t))))
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _hip.HipError("%s must be contiguous float32 (got %s, contiguous=%s)" % (name, t.dtype, t.is_contiguous()))
    return t


def _workspace(nbytes, device):
    """Scratch buffer; a fresh allocation keeps graph capture simple (the caching allocator pools it)."""
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _given_workspace(who, ws, ws_bytes, device):
    """The workspace operand of a call that needs ``ws_bytes`` (its ``*_ws_bytes`` query): a fresh one, or the caller's ``ws``
    (tests: a view between guard bands) after checking that it is a contiguous device tensor of at least that many bytes."""
    ws_bytes = int(ws_bytes)
    if ws is None:
        return _workspace(ws_bytes, device) if ws_bytes else None
    if not isinstance(ws, torch.Tensor) or not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < ws_bytes:
        raise _hip.HipError("%s: ws must be a contiguous device tensor of at least %d bytes" % (who, ws_bytes))
    return ws


def _given_output(who, out, shape, device, name="out"):
    """The result tensor of a call: a fresh one, or the caller's ``out`` (contiguous float32 on the device, of ``shape``)."""
    if out is None:
        return torch.empty(tuple(shape), dtype=torch.float32, device=device)
    _dev_f32(out, name)
    if tuple(out.shape) != tuple(shape):
        raise _hip.HipError("%s: %s has shape %s, expected %s" % (who, name, tuple(out.shape), tuple(shape)))
    return out


# what set_conv_autotune(True) means: 1 = every candidate plan is timed alone on an idle chip, 2 = under load (four launches
# of the candidate in flight on four streams: ranked by throughput, the objective of the four-frames-in-flight schedule)
AUTOTUNE_LEVEL = int(os.environ.get('FRCNN_AUTOTUNE_LEVEL', '2'))


def set_conv_autotune(enable):
    """Turn the convolution plan autotuner on/off (frcnn_conv2d_set_autotune): tune during eager warm-up frames,
    the cached plans are then used inside captured graphs.  ``True`` = AUTOTUNE_LEVEL; 1 / 2 select the level."""
    global _CONV_AUTOTUNE
    level = (AUTOTUNE_LEVEL if enable is True else int(enable)) if enable else 0
    _hip.check(_hip.load().frcnn_conv2d_set_autotune(level), "frcnn_conv2d_set_autotune")
    _CONV_AUTOTUNE = bool(enable)


def set_conv_algo(mode):
    """0 = the autotuner may choose Winograd F(2x2, 3x3) for the eligible 3x3 layers, 1 = implicit GEMM only,
    2 = Winograd wherever it applies (frcnn_conv2d_set_algo).  Flags: +16 never fuse the Winograd input transform into the
    64x64 GEMM's tile load, +32 forced Winograd (2) uses that fused form wherever C % 32 == 0 (tests), +128 Winograd never
    trims the transform components of partial tiles (odd map height / width) that feed only outputs outside the map - the
    default leaves them out in every mode, bit for bit the same result (A/B timing and tests; see ``winograd_rows``)."""
    global _CONV_ALGO_MODE, _CONV_ALGO_FLAGS
    _hip.check(_hip.load().frcnn_conv2d_set_algo(int(mode)), "frcnn_conv2d_set_algo")
    _CONV_ALGO_MODE = int(mode) & 3
    _CONV_ALGO_FLAGS = int(mode) & ~3


_CONV_ALGO_MODE = 0
_CONV_ALGO_FLAGS = 0
_CONV_AUTOTUNE = False


def conv_plan_algo(n, h, w, c, k, r, s, stride, pad, has_residual=False):
    """Form of the cached plan of this forward shape: -1 none, 0 implicit GEMM, 1 Winograd (frcnn_conv2d_plan_algo)."""
    return int(_hip.load().frcnn_conv2d_plan_algo(n, h, w, c, k, r, s, stride, pad, int(bool(has_residual))))


def winograd_filter_wanted(n, h, w, c, k, r, s, stride, pad):
    """Whether a residual-free call of this shape can read a pre-transformed Winograd filter NOW: its cached plan is a
    Winograd plan, or Winograd is forced (algo mode 2), or the shape is about to be tuned (autotune on, no plan yet: the tuner
    times the Winograd form too)."""
    if _CONV_ALGO_MODE == 1 or not winograd_eligible(k, r, s, c, stride, pad):
        return False
    if _CONV_ALGO_MODE == 2:
        return True
    algo = conv_plan_algo(n, h, w, c, k, r, s, stride, pad, False)
    return algo == 1 or (algo < 0 and _CONV_AUTOTUNE)


def winograd_rows(n, h, w):
    """(rows of the four component kinds, rows summed over the 16 components) that the grouped Winograd GEMM of an
    n x h x w map executes under the current ``set_conv_algo`` flags (frcnn_conv2d_winograd_rows; host only)."""
    out = (ctypes.c_long * 4)()
    total = _hip.load().frcnn_conv2d_winograd_rows(int(n), int(h), int(w), out)
    return [int(v) for v in out], int(total)


def conv_profile_begin():
    """Start per-dispatch timing of the convolution kernels (frcnn_conv2d_profile_begin)."""
    _hip.check(_hip.load().frcnn_conv2d_profile_begin(), "frcnn_conv2d_profile_begin")


def conv_profile_end(capacity=1 << 16):
    """Stop it; returns a list of (microseconds, conv2d_fwd call number, kind) per dispatch, kind 0 = main kernel,
    1 = split-K second pass."""
    us = (ctypes.c_float * capacity)()
    call = (ctypes.c_int * capacity)()
    kind = (ctypes.c_int * capacity)()
    n = _hip.load().frcnn_conv2d_profile_end(us, call, kind, capacity)
    if n > capacity:
        raise _hip.HipError("conv_profile_end: %d dispatches > capacity %d" % (n, capacity))
    return [(float(us[i]), int(call[i]), int(kind[i])) for i in range(n)]


def export_conv_plans():
    """The tuned convolution plans as a list of 13-int rows (frcnn_conv2d_export_plans)."""
    lib = _hip.load()
    n = lib.frcnn_conv2d_export_plans(None, 0)
    buf = (ctypes.c_int * (13 * max(n, 1)))()
    n = min(n, lib.frcnn_conv2d_export_plans(buf, n))
    return [[int(buf[13 * e + i]) for i in range(13)] for e in range(n)]


def import_conv_plans(rows):
    """Install plans saved by export_conv_plans (e.g. to profile exactly the kernels a timed run used)."""
    flat = [int(v) for row in rows for v in row]
    if len(flat) % 13:
        raise _hip.HipError("import_conv_plans: rows must have 13 ints")
    buf = (ctypes.c_int * max(len(flat), 1))(*flat)
    _hip.check(_hip.load().frcnn_conv2d_import_plans(buf, len(flat) // 13), "frcnn_conv2d_import_plans")


def conv_out_hw(h, w, r, s, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


def conv2d_nhwc(x, w_krsc, scale=None, shift=None, residual=None, stride=1, pad=0, relu=False, split_k=0, out=None,
                w_winograd=None, ws=None):
    """y = act(conv(x, w) * scale + shift + residual)  —  frcnn_conv2d_fwd (frcnn_conv2d_fwd_pre when the caller supplies
    the Winograd-transformed filter of a 3x3 / stride 1 / pad 1 layer, see ``winograd_filter``).  ``ws`` (tests): the
    workspace tensor to use, at least frcnn_conv2d_fwd_ws_bytes of it."""
    lib = _hip.load()
    _dev_f32(x, "x"); _dev_f32(w_krsc, "w")
    n, h, w, c = x.shape
    k, r, s, c2 = w_krsc.shape
    if c2 != c:
        raise _hip.HipError("conv2d_nhwc: input has %d channels, filter expects %d" % (c, c2))
    for nm, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _dev_f32(t, nm)
            if t.numel() != k:
                raise _hip.HipError("conv2d_nhwc: %s has %d elements, expected %d" % (nm, t.numel(), k))
    ho, wo = conv_out_hw(h, w, r, s, stride, pad)
    if out is None:
        out = torch.empty((n, ho, wo, k), dtype=torch.float32, device=x.device)
    else:
        _dev_f32(out, "out")
        if tuple(out.shape) != (n, ho, wo, k):
            raise _hip.HipError("conv2d_nhwc: out has shape %s, expected %s" % (tuple(out.shape), (n, ho, wo, k)))
    if residual is not None:
        _dev_f32(residual, "residual")
        if tuple(residual.shape) != (n, ho, wo, k):
            raise _hip.HipError("conv2d_nhwc: residual shape %s != output shape %s" % (tuple(residual.shape), (n, ho, wo, k)))
    ws_bytes = lib.frcnn_conv2d_fwd_ws_bytes(n, h, w, c, k, r, s, stride, pad, split_k)
    ws = _given_workspace("conv2d_nhwc", ws, ws_bytes, x.device)
    if w_winograd is not None:
        _dev_f32(w_winograd, "w_winograd")
        if tuple(w_winograd.shape) != (16, k, c):
            raise _hip.HipError("conv2d_nhwc: w_winograd has shape %s, expected %s" % (tuple(w_winograd.shape), (16, k, c)))
        _hip.check(lib.frcnn_conv2d_fwd_pre(_ptr(x), _ptr(w_krsc), _ptr(w_winograd), _ptr(scale), _ptr(shift), _ptr(residual),
                                            _ptr(out), n, h, w, c, k, r, s, stride, pad, int(bool(relu)), split_k, _ptr(ws),
                                            ws_bytes, _stream()), "frcnn_conv2d_fwd_pre")
    else:
        _hip.check(lib.frcnn_conv2d_fwd(_ptr(x), _ptr(w_krsc), _ptr(scale), _ptr(shift), _ptr(residual), _ptr(out), n, h, w,
                                        c, k, r, s, stride, pad, int(bool(relu)), split_k, _ptr(ws), ws_bytes, _stream()),
                   "frcnn_conv2d_fwd")
    if PROFILE is not None:
        PROFILE.append({"n": n, "h": h, "w": w, "c": c, "k": k, "r": r, "s": s, "stride": stride, "pad": pad,
                        "residual": residual is not None, "relu": bool(relu), "flops": 2.0 * n * ho * wo * k * r * s * c})
    if FLOPS is not None:
        _log_flops('fwd', 2.0 * n * ho * wo * k * r * s * c,
                   residual is None and winograd_eligible(k, r, s, c, stride, pad) and _CONV_ALGO_MODE != 1 and
                   (_CONV_ALGO_MODE == 2 or conv_plan_algo(n, h, w, c, k, r, s, stride, pad, False) == 1))
    return out


def conv2d_nhwc_winograd_res(x, w_krsc, residual, scale=None, shift=None, relu=False, out=None, w_winograd=None, ws=None):
    """y = act((conv3x3(x, w) * scale + shift) + residual) of a 3x3 / stride 1 / pad 1 layer (the closing convolution of a
    BasicBlock)  —  frcnn_conv2d_fwd_wres_pre: planned as the RESIDUAL-FREE call of its shape; where that plan is Winograd
    F(2x2, 3x3) the residual is added in the Winograd output transform (bit for bit the residual-free call with relu off, then a
    float32 add and a ReLU), otherwise the call is ``conv2d_nhwc(..., residual=residual)``.  ``w_winograd``: the pre-transformed
    filter (``winograd_filter``) or None; ``ws`` (tests): the workspace, frcnn_conv2d_fwd_ws_bytes of it."""
    lib = _hip.load()
    _dev_f32(x, "x"); _dev_f32(w_krsc, "w")
    if x.dim() != 4 or w_krsc.dim() != 4:
        raise _hip.HipError("conv2d_nhwc_winograd_res: x must be (n,h,w,c) and w (k,3,3,c), got %s and %s"
                            % (tuple(x.shape), tuple(w_krsc.shape)))
    n, h, w, c = x.shape
    k, r, s, c2 = w_krsc.shape
    if c2 != c:
        raise _hip.HipError("conv2d_nhwc_winograd_res: input has %d channels, filter expects %d" % (c, c2))
    if not winograd_eligible(k, r, s, c, 1, 1):
        raise _hip.HipError("conv2d_nhwc_winograd_res: need a (k,3,3,c) filter with k%%4 == 0 and c%%4 == 0, got %s" % (tuple(w_krsc.shape),))
    for nm, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _dev_f32(t, nm)
            if t.numel() != k:
                raise _hip.HipError("conv2d_nhwc_winograd_res: %s has %d elements, expected %d" % (nm, t.numel(), k))
    if residual is None:
        raise _hip.HipError("conv2d_nhwc_winograd_res: residual is None (conv2d_nhwc is the call without one)")
    _dev_f32(residual, "residual")
    if tuple(residual.shape) != (n, h, w, k):
        raise _hip.HipError("conv2d_nhwc_winograd_res: residual shape %s != output shape %s" % (tuple(residual.shape), (n, h, w, k)))
    out = _given_output("conv2d_nhwc_winograd_res", out, (n, h, w, k), x.device)
    if w_winograd is not None:
        _dev_f32(w_winograd, "w_winograd")
        if tuple(w_winograd.shape) != (16, k, c):
            raise _hip.HipError("conv2d_nhwc_winograd_res: w_winograd has shape %s, expected %s" % (tuple(w_winograd.shape), (16, k, c)))
    ws_bytes = lib.frcnn_conv2d_fwd_ws_bytes(n, h, w, c, k, 3, 3, 1, 1, 0)
    ws = _given_workspace("conv2d_nhwc_winograd_res", ws, ws_bytes, x.device)
    _hip.check(lib.frcnn_conv2d_fwd_wres_pre(_ptr(x), _ptr(w_krsc), _ptr(w_winograd), _ptr(scale), _ptr(shift), _ptr(residual),
                                             _ptr(out), n, h, w, c, k, 3, 3, 1, 1, int(bool(relu)), 0, _ptr(ws), ws_bytes,
                                             _stream()), "frcnn_conv2d_fwd_wres_pre")
    flops = 2.0 * n * h * w * k * 9 * c
    if PROFILE is not None:
        PROFILE.append({"n": n, "h": h, "w": w, "c": c, "k": k, "r": 3, "s": 3, "stride": 1, "pad": 1, "residual": True,
                        "relu": bool(relu), "flops": flops, "winograd_res": True})
    if FLOPS is not None:
        _log_flops('fwd', flops, _CONV_ALGO_MODE != 1 and (_CONV_ALGO_MODE == 2 or conv_plan_algo(n, h, w, c, k, 3, 3, 1, 1, False) == 1))
    return out


def conv2d_pack_bf16(w_krsc):
    """(K,R,S,C) fp32 filter -> the same array as bf16 words (int16 tensor), rounded to nearest even: the filter operand of
    ``conv2d_nhwc_bf16`` (frcnn_conv2d_pack_bf16); constant while the weights are."""
    _dev_f32(w_krsc, "w")
    if w_krsc.dim() != 4:
        raise _hip.HipError("conv2d_pack_bf16: need a (k,r,s,c) filter, got shape %s" % (tuple(w_krsc.shape),))
    lib = _hip.load()
    k, r, s, c = w_krsc.shape
    out = torch.empty((k, r, s, c), dtype=torch.int16, device=w_krsc.device)
    _hip.check(lib.frcnn_conv2d_pack_bf16(_ptr(w_krsc), _ptr(out), k, r, s, c, _stream()), "frcnn_conv2d_pack_bf16")
    return out


def set_conv_bf16_tile(mode):
    """Test / timing hook of ``conv2d_nhwc_bf16``: 0 = the library's rule, 1 = 64x64 tiles, 2 = 128x128 tiles
    (frcnn_conv2d_bf16_set_tile); the results do not depend on it."""
    _hip.check(_hip.load().frcnn_conv2d_bf16_set_tile(int(mode)), "frcnn_conv2d_bf16_set_tile")


def conv2d_nhwc_bf16(x, w_bf16, scale=None, shift=None, residual=None, stride=1, pad=0, relu=False, out=None):
    """y = act(conv(bf16(x), w_bf16) * scale + shift + residual) with fp32 accumulation  —  frcnn_conv2d_fwd_bf16.  x, scale,
    shift, residual and y are fp32 as for ``conv2d_nhwc``; ``w_bf16`` comes from ``conv2d_pack_bf16``.  Needs C % 32 == 0."""
    return _conv2d_nhwc_packed("conv2d_nhwc_bf16", "frcnn_conv2d_fwd_bf16", 1, x, w_bf16, scale, shift, residual, stride, pad, relu, out)


def conv2d_pack_bf16x3(w_krsc):
    """(K,R,S,C) fp32 filter -> (3,K,R,S,C) bf16 words (int16 tensor): hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid),
    round to nearest even, hi + mid + lo == w.  The filter operand of ``conv2d_nhwc_bf16x3`` (frcnn_conv2d_pack_bf16x3);
    constant while the weights are."""
    _dev_f32(w_krsc, "w")
    if w_krsc.dim() != 4:
        raise _hip.HipError("conv2d_pack_bf16x3: need a (k,r,s,c) filter, got shape %s" % (tuple(w_krsc.shape),))
    lib = _hip.load()
    k, r, s, c = w_krsc.shape
    out = torch.empty((3, k, r, s, c), dtype=torch.int16, device=w_krsc.device)
    _hip.check(lib.frcnn_conv2d_pack_bf16x3(_ptr(w_krsc), _ptr(out), k, r, s, c, _stream()), "frcnn_conv2d_pack_bf16x3")
    return out


def conv2d_nhwc_bf16x3(x, w_bf16x3, scale=None, shift=None, residual=None, stride=1, pad=0, relu=False, out=None):
    """y = act(conv(x, w) * scale + shift + residual) to fp32 accuracy on the bf16 matrix pipe  —  frcnn_conv2d_fwd_bf16x3:
    every product as six bf16 products of the operands' hi / mid / lo planes, fp32 accumulation.  ``w_bf16x3`` comes from
    ``conv2d_pack_bf16x3``.  Needs C % 32 == 0; for finite operands below about 2^120 (an infinite operand gives NaN)."""
    return _conv2d_nhwc_packed("conv2d_nhwc_bf16x3", "frcnn_conv2d_fwd_bf16x3", 3, x, w_bf16x3, scale, shift, residual, stride, pad, relu, out)


def conv_split_bf16_wanted(n, h, w, c, k, r, s, stride, pad):
    """Does the library's rule give this convolution to the split-bf16 kernel (frcnn_conv2d_split_bf16_wanted)?  False
    while a hook pins the fp32 kernels - a forced tile, ``set_conv_algo`` (mode or flags) or the staging mode away from
    their defaults - and after ``frcnn_conv2d_split_bf16_enable(0)``.  An imported plan table does not pin it."""
    args = [int(v) for v in (n, h, w, c, k, r, s, stride, pad)]
    if min(args[:8]) < 1 or args[8] < 0:
        raise _hip.HipError("conv_split_bf16_wanted: bad geometry n=%d h=%d w=%d c=%d k=%d r=%d s=%d stride=%d pad=%d" % tuple(args))
    return bool(_hip.load().frcnn_conv2d_split_bf16_wanted(*args))


def _conv2d_nhwc_packed(what, entry, planes, x, w_bf16, scale, shift, residual, stride, pad, relu, out):
    """The bf16-operand wrappers' common body: ``w_bf16`` is (k,r,s,c) for one plane, (3,k,r,s,c) for the split form."""
    _dev_f32(x, "x")
    if not isinstance(w_bf16, torch.Tensor) or not w_bf16.is_cuda:
        raise _hip.HipError("w_bf16 must be a tensor on the MI355X (got %s); this package has no CPU path"
                            % (getattr(w_bf16, "device", type(w_bf16)),))
    layout, packer = ("(k,r,s,c)", "conv2d_pack_bf16") if planes == 1 else ("(3,k,r,s,c)", "conv2d_pack_bf16x3")
    if (w_bf16.dtype != torch.int16 or not w_bf16.is_contiguous() or w_bf16.dim() != (4 if planes == 1 else 5)
            or (planes != 1 and w_bf16.shape[0] != planes)):
        raise _hip.HipError("w_bf16 must be a contiguous %s int16 tensor of bf16 words (%s), got %s %s"
                            % (layout, packer, w_bf16.dtype, tuple(w_bf16.shape)))
    if x.dim() != 4:
        raise _hip.HipError("%s: x must be (n,h,w,c), got shape %s" % (what, tuple(x.shape)))
    n, h, w, c = x.shape
    k, r, s, c2 = w_bf16.shape[-4:]
    if c2 != c:
        raise _hip.HipError("%s: input has %d channels, filter expects %d" % (what, c, c2))
    if c % 32 != 0:
        raise _hip.HipError("%s: needs c %% 32 == 0, got c = %d" % (what, c))
    stride, pad = int(stride), int(pad)
    if stride < 1 or pad < 0 or h + 2 * pad < r or w + 2 * pad < s:
        raise _hip.HipError("%s: bad geometry h=%d w=%d r=%d s=%d stride=%d pad=%d" % (what, h, w, r, s, stride, pad))
    for nm, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _dev_f32(t, nm)
            if t.numel() != k:
                raise _hip.HipError("%s: %s has %d elements, expected %d" % (what, nm, t.numel(), k))
    ho, wo = conv_out_hw(h, w, r, s, stride, pad)
    if out is None:
        out = torch.empty((n, ho, wo, k), dtype=torch.float32, device=x.device)
    else:
        _dev_f32(out, "out")
        if tuple(out.shape) != (n, ho, wo, k):
            raise _hip.HipError("%s: out has shape %s, expected %s" % (what, tuple(out.shape), (n, ho, wo, k)))
    if residual is not None:
        _dev_f32(residual, "residual")
        if tuple(residual.shape) != (n, ho, wo, k):
            raise _hip.HipError("%s: residual shape %s != output shape %s" % (what, tuple(residual.shape), (n, ho, wo, k)))
    _hip.check(getattr(_hip.load(), entry)(_ptr(x), _ptr(w_bf16), _ptr(scale), _ptr(shift), _ptr(residual), _ptr(out), n, h,
                                           w, c, k, r, s, stride, pad, int(bool(relu)), _stream()), entry)
    if PROFILE is not None:
        PROFILE.append({"n": n, "h": h, "w": w, "c": c, "k": k, "r": r, "s": s, "stride": stride, "pad": pad,
                        "residual": residual is not None, "relu": bool(relu), "flops": 2.0 * n * ho * wo * k * r * s * c,
                        ("bf16" if planes == 1 else "split_bf16"): True})
    if FLOPS is not None:
        _log_flops('fwd', 2.0 * n * ho * wo * k * r * s * c)
    return out


def winograd_eligible(k, r, s, c, stride, pad):
    """The layers frcnn_conv2d_set_algo's Winograd F(2x2, 3x3) form applies to (no residual operand)."""
    return r == 3 and s == 3 and stride == 1 and pad == 1 and c % 4 == 0 and k % 4 == 0


def winograd_filter(w_krsc):
    """(K,3,3,C) filter -> its Winograd transform U (16,K,C) (frcnn_conv2d_winograd_filter); constant while the weights are."""
    lib = _hip.load()
    _dev_f32(w_krsc, "w")
    k, r, s, c = w_krsc.shape
    if not winograd_eligible(k, r, s, c, 1, 1):
        raise _hip.HipError("winograd_filter: need a (k,3,3,c) filter with k%4 == 0 and c%4 == 0")
    u = torch.empty((16, k, c), dtype=torch.float32, device=w_krsc.device)
    _hip.check(lib.frcnn_conv2d_winograd_filter(_ptr(w_krsc), _ptr(u), k, c, _stream()), "frcnn_conv2d_winograd_filter")
    return u


def conv2d_transpose_filter(w_krsc):
    """(K,R,S,C) -> (C,R,S,K) with flipped taps: the filter of the data-gradient convolution."""
    lib = _hip.load()
    _dev_f32(w_krsc, "w")
    k, r, s, c = w_krsc.shape
    out = torch.empty((c, r, s, k), dtype=torch.float32, device=w_krsc.device)
    _hip.check(lib.frcnn_conv2d_transpose_filter(_ptr(w_krsc), _ptr(out), k, r, s, c, _stream()),
               "frcnn_conv2d_transpose_filter")
    return out


def dgrad_winograd_wanted(x_shape, k, r, s, stride, pad):
    """Whether the data-gradient convolution of this layer (a stride-1 3x3 convolution of dy with the transposed filter) can
    read a pre-transformed Winograd filter now (see ``winograd_filter_wanted``)."""
    n, h, w, c = x_shape
    if stride != 1 or r != 3 or s != 3 or r - 1 - pad != 1:
        return False
    ho, wo = conv_out_hw(h, w, r, s, stride, pad)
    return winograd_filter_wanted(n, ho, wo, k, c, r, s, 1, 1)


def conv2d_bwd_data(dy, w_t, x_shape, stride=1, pad=0, add=None, w_winograd=None, act_y=None, act_scale=None, out=None, ws=None):
    """dx (n,h,w,c) = conv_transpose(dy, w) [+ add].  w_t = conv2d_transpose_filter(w); x_shape = forward input shape.
    ``w_winograd`` = winograd_filter(w_t) (16, c, k): frcnn_conv2d_bwd_data_pre.  ``act_y`` (shape of dx) [, ``act_scale``
    (c,)]: the result is masked / scaled like ``act_bwd(dx, act_y, act_scale, relu=True)`` would in a second pass
    (frcnn_conv2d_bwd_data_act; not for the strided 1x1 form).  ``out`` / ``ws`` (tests): the result / workspace tensor to use."""
    lib = _hip.load()
    _dev_f32(dy, "dy"); _dev_f32(w_t, "w_t")
    n, h, w, c = x_shape
    c2, r, s, k = w_t.shape
    if c2 != c or dy.shape[-1] != k:
        raise _hip.HipError("conv2d_bwd_data: filter (C=%d,K=%d) does not match x C=%d / dy K=%d" % (c2, k, c, dy.shape[-1]))
    if tuple(dy.shape[:3]) != (n,) + conv_out_hw(h, w, r, s, stride, pad):
        raise _hip.HipError("conv2d_bwd_data: dy shape %s does not match the forward output" % (tuple(dy.shape),))
    if add is not None:
        _dev_f32(add, "add")
        if tuple(add.shape) != tuple(x_shape):
            raise _hip.HipError("conv2d_bwd_data: add shape %s != x shape %s" % (tuple(add.shape), tuple(x_shape)))
    dx = _given_output("conv2d_bwd_data", out, x_shape, dy.device)
    if FLOPS is not None:
        _log_flops('dgrad', 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * k * r * s * c,
                   add is None and dgrad_winograd_wanted(x_shape, k, r, s, stride, pad))
    ws_bytes = lib.frcnn_conv2d_bwd_data_ws_bytes(n, h, w, c, k, r, s, stride, pad)
    ws = _given_workspace("conv2d_bwd_data", ws, ws_bytes, dy.device)
    if act_y is not None:
        _dev_f32(act_y, "act_y")
        if tuple(act_y.shape) != tuple(x_shape):
            raise _hip.HipError("conv2d_bwd_data: act_y shape %s != x shape %s" % (tuple(act_y.shape), tuple(x_shape)))
        if act_scale is not None:
            _dev_f32(act_scale, "act_scale")
            if act_scale.numel() != c:
                raise _hip.HipError("conv2d_bwd_data: act_scale has %d elements, expected %d" % (act_scale.numel(), c))
        if w_winograd is not None:
            _dev_f32(w_winograd, "w_winograd")
            if tuple(w_winograd.shape) != (16, c, k) or add is not None:
                w_winograd = None
        _hip.check(lib.frcnn_conv2d_bwd_data_act(_ptr(dy), _ptr(w_t), _ptr(w_winograd), _ptr(add), _ptr(act_y), _ptr(act_scale),
                                                 _ptr(dx), n, h, w, c, k, r, s, stride, pad, _ptr(ws), ws_bytes, _stream()),
                   "frcnn_conv2d_bwd_data_act")
        return dx
    if w_winograd is not None and add is None:
        _dev_f32(w_winograd, "w_winograd")
        if tuple(w_winograd.shape) != (16, c, k):
            raise _hip.HipError("conv2d_bwd_data: w_winograd has shape %s, expected %s" % (tuple(w_winograd.shape), (16, c, k)))
        _hip.check(lib.frcnn_conv2d_bwd_data_pre(_ptr(dy), _ptr(w_t), _ptr(w_winograd), None, _ptr(dx), n, h, w, c, k, r, s,
                                                 stride, pad, _ptr(ws), ws_bytes, _stream()), "frcnn_conv2d_bwd_data_pre")
        return dx
    _hip.check(lib.frcnn_conv2d_bwd_data(_ptr(dy), _ptr(w_t), _ptr(add), _ptr(dx), n, h, w, c, k, r, s, stride, pad,
                                         _ptr(ws), ws_bytes, _stream()), "frcnn_conv2d_bwd_data")
    return dx


# Tile counters of the filter-gradient and BatchNorm kernels (`counters` of frcnn_conv2d_bwd_weight[_acc], frcnn_bn_train_fwd /
# _bwd: the last workgroup of a tile / column block finishes the reduction): device ints that are zero when a
# launch starts and zero again when it ends; launches that may be in flight together must not share them.
#   * eager launches take consecutive ranges of a per-device ring: a range comes round again only after WGRAD_COUNTER_RING
#     ints of later launches - far more launches than can be in flight;
#   * a holder of a captured graph installs its OWN arena for its warm-up and capture (``wgrad_counter_arena``; the ranges
#     are baked into the graph, and no other graph or eager launch ever gets them) and rewinds it at the start of every
#     pass over its launch sequence;
#   * a capture WITHOUT an arena zero-fills fresh counters inside the capture (private to the graph, one fill kernel per call).
WGRAD_COUNTER_RING = 1 << 20
_COUNTER_RINGS = {}
WGRAD_ARENA = None


class CounterArena:
    def __init__(self, device, count=1 << 19):
        self.ints = torch.zeros(int(count), dtype=torch.int32, device=device)
        self.cursor = 0

    def rewind(self):
        self.cursor = 0

    def take(self, count):
        if self.cursor + count > self.ints.numel():
            raise _hip.HipError("filter-gradient counter arena exhausted (%d + %d > %d ints)" % (self.cursor, count, self.ints.numel()))
        start = self.cursor
        self.cursor += count
        return self.ints[start:start + count]


class wgrad_counter_arena:
    """``with ops.wgrad_counter_arena(arena):`` - filter-gradient launches inside take their tile counters from ``arena``."""

    def __init__(self, arena):
        self.arena = arena

    def __enter__(self):
        global WGRAD_ARENA
        self.prev, WGRAD_ARENA = WGRAD_ARENA, self.arena
        return self.arena

    def __exit__(self, *exc):
        global WGRAD_ARENA
        WGRAD_ARENA = self.prev
        return False


def _tile_counters(device, count):
    if WGRAD_ARENA is not None:
        if WGRAD_ARENA.ints.device != device:
            raise _hip.HipError("filter-gradient counter arena is on %s, the launch on %s" % (WGRAD_ARENA.ints.device, device))
        return WGRAD_ARENA.take(count)
    if torch.device(device).type == 'cuda' and torch.cuda.is_current_stream_capturing():
        return torch.zeros(count, dtype=torch.int32, device=device)
    ring = _COUNTER_RINGS.get(str(device))
    if ring is None:
        ring = _COUNTER_RINGS[str(device)] = CounterArena(device, WGRAD_COUNTER_RING)
    if ring.cursor + count > ring.ints.numel():
        ring.rewind()
    return ring.take(count)


def set_wgrad_variant(variant):
    """frcnn_conv2d_wgrad_set_variant: 0 every filter-gradient kernel, 1 register-staged only, 2 LDS-DMA wherever it applies."""
    _hip.check(_hip.load().frcnn_conv2d_wgrad_set_variant(int(variant)), "frcnn_conv2d_wgrad_set_variant")


def set_wgrad_plan(kernel, splits=1):
    """frcnn_conv2d_wgrad_set_plan: force (kernel 1..4, pixel splits) for every following filter gradient; kernel 0 = off."""
    _hip.check(_hip.load().frcnn_conv2d_wgrad_set_plan(int(kernel), int(splits)), "frcnn_conv2d_wgrad_set_plan")


def _wgrad_operands(who, x, dy, r, s, stride, pad, grad_w=None):
    """What the filter-gradient wrappers check and log alike: the operands on the device, dy against the forward output's
    shape, grad_w against (k, c_real <= c, r, s), the call's direct-form FLOPs.  Returns (n, h, w, c, k, c_real)."""
    _dev_f32(x, "x"); _dev_f32(dy, "dy")
    n, h, w, c = x.shape
    k = dy.shape[-1]
    if tuple(dy.shape[:3]) != (n,) + conv_out_hw(h, w, r, s, stride, pad):
        raise _hip.HipError("%s: dy shape %s does not match the forward output" % (who, tuple(dy.shape)))
    c_real = c
    if grad_w is not None:
        _dev_f32(grad_w, "grad_w")
        c_real = grad_w.shape[1]
        if grad_w.shape[0] != k or c_real > c or grad_w.numel() != k * c_real * r * s:
            raise _hip.HipError("%s: grad_w %s does not fit k=%d c<=%d r=%d s=%d" % (who, tuple(grad_w.shape), k, c, r, s))
    _log_flops('wgrad', 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * k * r * s * c)
    return n, h, w, c, k, c_real


def _wgrad_scratch(who, lib, device, n, h, w, c, k, r, s, stride, pad, ws=None):
    """(workspace, its bytes, tile counters) of one frcnn_conv2d_bwd_weight[_acc] call"""
    ws_bytes = lib.frcnn_conv2d_bwd_weight_ws_bytes(n, h, w, c, k, r, s, stride, pad)
    ws = _given_workspace(who, ws, ws_bytes, device)
    return ws, ws_bytes, _tile_counters(device, lib.frcnn_conv2d_bwd_weight_counters(c, k, r, s))


def conv2d_bwd_weight(x, dy, r, s, stride=1, pad=0, want_bias=False, out=None, out_bias=None, ws=None):
    """Returns (dw (K,R,S,C), db (K,) or None).  ``out`` / ``out_bias`` / ``ws`` (tests): the dw / db / workspace tensor to use."""
    lib = _hip.load()
    n, h, w, c, k, _ = _wgrad_operands("conv2d_bwd_weight", x, dy, r, s, stride, pad)
    dw = _given_output("conv2d_bwd_weight", out, (k, r, s, c), x.device)
    db = _given_output("conv2d_bwd_weight", out_bias, (k,), x.device, "out_bias") if want_bias else None
    ws, ws_bytes, counters = _wgrad_scratch("conv2d_bwd_weight", lib, x.device, n, h, w, c, k, r, s, stride, pad, ws)
    _hip.check(lib.frcnn_conv2d_bwd_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), n, h, w, c, k, r, s, stride, pad,
                                           _ptr(ws), ws_bytes, counters.data_ptr(), _stream()), "frcnn_conv2d_bwd_weight")
    return dw, db


def conv2d_bwd_weight_acc(x, dy, r, s, grad_w, grad_b=None, stride=1, pad=0, ws=None):
    """grad_w (K, C_real, R, S) [or (K, C_real) with r = s = 1] += filter gradient, grad_b (K,) += bias gradient: the
    parameter's own gradient buffers, accumulated in place (frcnn_conv2d_bwd_weight_acc; the results are ``grad_w`` / ``grad_b``
    themselves, so there is no ``out``).  ``ws`` (tests): the workspace tensor to use."""
    lib = _hip.load()
    n, h, w, c, k, c_real = _wgrad_operands("conv2d_bwd_weight_acc", x, dy, r, s, stride, pad, grad_w)
    if grad_b is not None:
        _dev_f32(grad_b, "grad_b")
    ws, ws_bytes, counters = _wgrad_scratch("conv2d_bwd_weight_acc", lib, x.device, n, h, w, c, k, r, s, stride, pad, ws)
    _hip.check(lib.frcnn_conv2d_bwd_weight_acc(_ptr(x), _ptr(dy), _ptr(grad_w), c_real, _ptr(grad_b), n, h, w, c, k, r, s,
                                               stride, pad, _ptr(ws), ws_bytes, counters.data_ptr(), _stream()),
               "frcnn_conv2d_bwd_weight_acc")


def _packed_bf16(who, name, t, shape):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _hip.HipError("%s must be a tensor on the MI355X (got %s); this package has no CPU path"
                            % (name, getattr(t, "device", type(t))))
    if t.dtype != torch.int16 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise _hip.HipError("%s: %s must be a contiguous %s int16 tensor of bf16 words (conv2d_pack_bf16), got %s %s"
                            % (who, name, tuple(shape), t.dtype, tuple(t.shape)))


def conv2d_bwd_data_bf16(dy, w_t_bf16, x_shape, stride=1, pad=0, add=None, act_y=None, act_scale=None, out=None, ws=None):
    """dx (n,h,w,c) = act_bwd(conv_transpose(bf16(dy), w) [+ add]) with bf16 products and fp32 accumulation  -
    frcnn_conv2d_bwd_data_bf16: what ``conv2d_bwd_data`` computes, ``add`` / ``act_y`` / ``act_scale`` included, for the stride-1
    form and the zero-inserted strided r x s form.  ``w_t_bf16`` = conv2d_pack_bf16(conv2d_transpose_filter(w)), (c,r,s,k);
    needs k % 32 == 0.  The strided 1x1 form (scattered output) has no bf16 form and raises.  ``out`` / ``ws`` (tests): the result /
    workspace tensor to use."""
    lib = _hip.load()
    who = "conv2d_bwd_data_bf16"
    _dev_f32(dy, "dy")
    n, h, w, c = [int(v) for v in x_shape]
    if dy.dim() != 4 or not isinstance(w_t_bf16, torch.Tensor) or w_t_bf16.dim() != 4:
        raise _hip.HipError("%s: dy must be (n,ho,wo,k) and w_t_bf16 (c,r,s,k)" % who)
    _, r, s, k = w_t_bf16.shape
    _packed_bf16(who, "w_t_bf16", w_t_bf16, (c, r, s, dy.shape[-1]))
    stride, pad = int(stride), int(pad)
    if k % 32 != 0 or c % 4 != 0:
        raise _hip.HipError("%s: needs k %% 32 == 0 and c %% 4 == 0, got k = %d, c = %d" % (who, k, c))
    if stride > 1 and r == 1 and s == 1:
        raise _hip.HipError("%s: the strided 1x1 data gradient (scattered output) has no bf16 form" % who)
    if stride < 1 or pad < 0 or h + 2 * pad < r or w + 2 * pad < s or tuple(dy.shape[:3]) != (n,) + conv_out_hw(h, w, r, s, stride, pad):
        raise _hip.HipError("%s: dy shape %s does not match the forward output" % (who, tuple(dy.shape)))
    for nm, t in (("add", add), ("act_y", act_y)):
        if t is not None:
            _dev_f32(t, nm)
            if tuple(t.shape) != (n, h, w, c):
                raise _hip.HipError("%s: %s shape %s != x shape %s" % (who, nm, tuple(t.shape), (n, h, w, c)))
    if act_scale is not None:
        _dev_f32(act_scale, "act_scale")
        if act_y is None or act_scale.numel() != c:
            raise _hip.HipError("%s: act_scale needs act_y and %d elements" % (who, c))
    dx = _given_output(who, out, (n, h, w, c), dy.device)
    if FLOPS is not None:
        _log_flops('dgrad', 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * k * r * s * c)
    ws_bytes = lib.frcnn_conv2d_bwd_data_bf16_ws_bytes(n, h, w, c, k, r, s, stride, pad)
    ws = _given_workspace(who, ws, ws_bytes, dy.device)
    _hip.check(lib.frcnn_conv2d_bwd_data_bf16(_ptr(dy), _ptr(w_t_bf16), _ptr(add), _ptr(act_y), _ptr(act_scale), _ptr(dx), n, h, w, c,
                                              k, r, s, stride, pad, _ptr(ws), ws_bytes, _stream()), "frcnn_conv2d_bwd_data_bf16")
    return dx


def conv2d_bwd_weight_bf16_ws_bytes(x_shape, k, r, s, stride=1, pad=0, splits=0):
    """Workspace bytes of ``conv2d_bwd_weight_bf16`` / ``conv2d_bwd_weight_acc_bf16`` for this shape and split count."""
    n, h, w, c = [int(v) for v in x_shape]
    return int(_hip.load().frcnn_conv2d_bwd_weight_bf16_ws_bytes(n, h, w, c, int(k), int(r), int(s), int(stride), int(pad), int(splits)))


def _wgrad_bf16_ws(who, device, n, h, w, c, k, r, s, stride, pad, splits, ws):
    splits = int(splits)
    if splits < 0:
        raise _hip.HipError("%s: splits must be >= 0 (0 = the library's choice), got %d" % (who, splits))
    ws_bytes = conv2d_bwd_weight_bf16_ws_bytes((n, h, w, c), k, r, s, stride, pad, splits)
    return splits, _given_workspace(who, ws, ws_bytes, device), ws_bytes


def conv2d_bwd_weight_bf16(x, dy, r, s, stride=1, pad=0, want_bias=False, splits=0, out=None, ws=None):
    """(dw (K,R,S,C), db (K,) or None): dw = sum over pixels of bf16(dy) * bf16(patch(x)), fp32 accumulation
    (frcnn_conv2d_bwd_weight_bf16); db in fp32.  ``splits``: pixel ranges whose fp32 partial sums are added in order (0 = the
    library's choice; clamped to the number of 32-pixel steps); ``out`` / ``ws`` (tests): the result / workspace tensor to use."""
    lib = _hip.load()
    n, h, w, c, k, _ = _wgrad_operands("conv2d_bwd_weight_bf16", x, dy, r, s, stride, pad)
    out = _given_output("conv2d_bwd_weight_bf16", out, (k, r, s, c), x.device)
    db = torch.empty((k,), dtype=torch.float32, device=x.device) if want_bias else None
    splits, ws, ws_bytes = _wgrad_bf16_ws("conv2d_bwd_weight_bf16", x.device, n, h, w, c, k, r, s, stride, pad, splits, ws)
    _hip.check(lib.frcnn_conv2d_bwd_weight_bf16(_ptr(x), _ptr(dy), _ptr(out), _ptr(db), n, h, w, c, k, r, s, stride, pad, splits,
                                                _ptr(ws), ws_bytes, _stream()), "frcnn_conv2d_bwd_weight_bf16")
    return out, db


def conv2d_bwd_weight_acc_bf16(x, dy, r, s, grad_w, grad_b=None, stride=1, pad=0, splits=0, ws=None):
    """grad_w (K, C_real, R, S) += the bf16-operand filter gradient, grad_b (K,) += the fp32 bias gradient, in place
    (frcnn_conv2d_bwd_weight_acc_bf16); ``splits`` / ``ws`` as for ``conv2d_bwd_weight_bf16``."""
    lib = _hip.load()
    n, h, w, c, k, c_real = _wgrad_operands("conv2d_bwd_weight_acc_bf16", x, dy, r, s, stride, pad, grad_w)
    if grad_b is not None:
        _dev_f32(grad_b, "grad_b")
    splits, ws, ws_bytes = _wgrad_bf16_ws("conv2d_bwd_weight_acc_bf16", x.device, n, h, w, c, k, r, s, stride, pad, splits, ws)
    _hip.check(lib.frcnn_conv2d_bwd_weight_acc_bf16(_ptr(x), _ptr(dy), _ptr(grad_w), c_real, _ptr(grad_b), n, h, w, c, k, r, s,
                                                    stride, pad, splits, _ptr(ws), ws_bytes, _stream()),
               "frcnn_conv2d_bwd_weight_acc_bf16")


WGRAD_MAX_GROUPS = 24


def conv2d_bwd_weight_acc_grouped(xs, dys, r, s, grads, stride=1, pad=0, ws=None):
    """``grads[g]`` += filter gradient of convolution g for up to WGRAD_MAX_GROUPS convolutions of identical shape
    (frcnn_conv2d_bwd_weight_acc_grouped): one launch pair, no pixel split, no slab reduction.  ``ws`` (tests): the workspace
    tensor to use."""
    import ctypes
    lib = _hip.load()
    groups = len(xs)
    if not (0 < groups <= WGRAD_MAX_GROUPS) or len(dys) != groups or len(grads) != groups:
        raise _hip.HipError("conv2d_bwd_weight_acc_grouped: 1..%d groups, same number of x / dy / grad tensors" % WGRAD_MAX_GROUPS)
    who = "conv2d_bwd_weight_acc_grouped"
    first = None
    for x, dy, gw in zip(xs, dys, grads):
        if x.shape != xs[0].shape or dy.shape != dys[0].shape:
            raise _hip.HipError("%s: every group must have the shape of the first" % who)
        n, h, w, c, k, c_real = _wgrad_operands(who, x, dy, r, s, stride, pad, gw)
        first = first or c_real
        if c_real != first:
            raise _hip.HipError("%s: grad_w %s does not fit k=%d c<=%d r=%d s=%d" % (who, tuple(gw.shape), k, c, r, s))
    arr = ctypes.c_void_p * groups
    ws_bytes = lib.frcnn_conv2d_bwd_weight_acc_grouped_ws_bytes(groups, c, k, r, s)
    ws = _given_workspace("conv2d_bwd_weight_acc_grouped", ws, ws_bytes, xs[0].device)
    _hip.check(lib.frcnn_conv2d_bwd_weight_acc_grouped(arr(*[t.data_ptr() for t in xs]), arr(*[t.data_ptr() for t in dys]),
                                                       arr(*[t.data_ptr() for t in grads]), groups, c_real, n, h, w, c, k, r, s,
                                                       stride, pad, _ptr(ws), ws_bytes, _stream()),
               "frcnn_conv2d_bwd_weight_acc_grouped")


def maxpool3x3s2_nhwc(x):
    lib = _hip.load()
    _dev_f32(x, "x")
    n, h, w, c = x.shape
    out = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=torch.float32, device=x.device)
    _hip.check(lib.frcnn_maxpool3x3s2_fwd(_ptr(x), _ptr(out), n, h, w, c, _stream()), "frcnn_maxpool3x3s2_fwd")
    return out


def maxpool3x3s2_bwd(x, dy):
    """Backward of maxpool3x3s2_nhwc: x (N,H,W,C) the pooled input, dy (N,Ho,Wo,C) -> dx like x."""
    lib = _hip.load()
    _dev_f32(x, "x"); _dev_f32(dy, "dy")
    n, h, w, c = x.shape
    if tuple(dy.shape) != (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c):
        raise _hip.HipError("maxpool3x3s2_bwd: dy %s does not match x %s" % (tuple(dy.shape), tuple(x.shape)))
    dx = torch.empty_like(x)
    _hip.check(lib.frcnn_maxpool3x3s2_bwd(_ptr(x), _ptr(dy), _ptr(dx), n, h, w, c, _stream()), "frcnn_maxpool3x3s2_bwd")
    return dx


# frcnn_maxpool2x2s2_fwd: the most lanes one launch has (include/frcnn_hip.h FRCNN_MAXPOOL2X2_MAX_LANES); more work items
# than this make every lane walk its loop more than once
MAXPOOL2X2_MAX_LANES = 2048 * 256


def maxpool2x2s2_nhwc(x, out=None):
    """nn.MaxPool2d(kernel_size=2, stride=2) (ceil_mode off; lib/nets/vgg16.py:35,46) on an NHWC fp32 tensor
    (frcnn_maxpool2x2s2_fwd): x (N,H,W,C), C % 4 == 0 -> (N, H // 2, W // 2, C).  The trailing row / column of an odd H / W is
    never read; a NaN in a window gives NaN, as torch does.  ``out``: a tensor of the result's shape to write into."""
    lib = _hip.load()
    _dev_f32(x, "maxpool2x2s2_nhwc: x")
    if x.dim() != 4:
        raise _hip.HipError("maxpool2x2s2_nhwc: x must be (N,H,W,C), got %s" % (tuple(x.shape),))
    n, h, w, c = x.shape
    shape = (n, h // 2, w // 2, c)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _dev_f32(out, "maxpool2x2s2_nhwc: out")
        if tuple(out.shape) != shape or out.device != x.device:
            raise _hip.HipError("maxpool2x2s2_nhwc: out must be %s on %s, got %s" % (shape, x.device, tuple(out.shape)))
    _hip.check(lib.frcnn_maxpool2x2s2_fwd(_ptr(x), _ptr(out), n, h, w, c, _stream()), "frcnn_maxpool2x2s2_fwd")
    return out


def maxpool2x2s2_bwd(x, dy, relu=False, out=None):
    """Backward of maxpool2x2s2_nhwc (frcnn_maxpool2x2s2_bwd): x (N,H,W,C) the pooled input, dy (N, H // 2, W // 2, C) -> dx
    like x.  Per window torch's winner receives dy, everything else - the trailing row / column of an odd H / W included -
    0: the launch writes every element of dx.  ``relu``: x is a ReLU output and dx the gradient of the ReLU's input (the
    winner receives dy only if it is > 0), which saves the act_bwd pass.  ``out``: a tensor of x's shape to write into."""
    lib = _hip.load()
    _dev_f32(x, "maxpool2x2s2_bwd: x")
    _dev_f32(dy, "maxpool2x2s2_bwd: dy")
    if x.dim() != 4:
        raise _hip.HipError("maxpool2x2s2_bwd: x must be (N,H,W,C), got %s" % (tuple(x.shape),))
    n, h, w, c = x.shape
    if tuple(dy.shape) != (n, h // 2, w // 2, c) or dy.device != x.device:
        raise _hip.HipError("maxpool2x2s2_bwd: dy must be %s on %s, got %s" % ((n, h // 2, w // 2, c), x.device, tuple(dy.shape)))
    if out is None:
        out = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    else:
        _dev_f32(out, "maxpool2x2s2_bwd: out")
        if tuple(out.shape) != tuple(x.shape) or out.device != x.device:
            raise _hip.HipError("maxpool2x2s2_bwd: out must be %s on %s, got %s" % (tuple(x.shape), x.device, tuple(out.shape)))
    _hip.check(lib.frcnn_maxpool2x2s2_bwd(_ptr(x), _ptr(dy), _ptr(out), n, h, w, c, int(bool(relu)), _stream()),
               "frcnn_maxpool2x2s2_bwd")
    return out


# frcnn_dwconv3x3_fwd: outputs along W one lane produces per work item (include/frcnn_hip.h FRCNN_DWCONV_STRIP)
DWCONV_STRIP = 4


def depthwise_conv3x3_nhwc(x, w_rsc, scale=None, shift=None, stride=1, relu=False, in_cap=float('inf'),
                           out_cap=float('inf'), out=None):
    """Depthwise 3x3 / pad 1 convolution with a per-channel affine epilogue (frcnn_dwconv3x3_fwd; MobileNet-v1's conv_dw,
    lib/nets/mobilenet_v1.py:117-123): x (N,H,W,C), w_rsc (3,3,C), scale / shift (C,) or None ->
    min(act(conv(min(x, in_cap)) * scale + shift), out_cap), (N,OH,OW,C).  ``out``: a tensor of that shape to write into."""
    lib = _hip.load()
    _dev_f32(x, "depthwise_conv3x3_nhwc: x")
    _dev_f32(w_rsc, "depthwise_conv3x3_nhwc: w_rsc")
    if x.dim() != 4:
        raise _hip.HipError("depthwise_conv3x3_nhwc: x must be (N,H,W,C), got %s" % (tuple(x.shape),))
    n, h, w, c = x.shape
    if tuple(w_rsc.shape) != (3, 3, c) or w_rsc.device != x.device:
        raise _hip.HipError("depthwise_conv3x3_nhwc: w_rsc must be (3,3,%d) on %s, got %s" % (c, x.device, tuple(w_rsc.shape)))
    for t, name in ((scale, "scale"), (shift, "shift")):
        if t is not None:
            _dev_f32(t, "depthwise_conv3x3_nhwc: " + name)
            if tuple(t.shape) != (c,) or t.device != x.device:
                raise _hip.HipError("depthwise_conv3x3_nhwc: %s must be (%d,) on %s, got %s" % (name, c, x.device, tuple(t.shape)))
    stride = int(stride)
    if stride not in (1, 2):
        raise _hip.HipError("depthwise_conv3x3_nhwc: stride %d (1 or 2)" % stride)
    shape = (n, (h - 1) // stride + 1, (w - 1) // stride + 1, c)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _dev_f32(out, "depthwise_conv3x3_nhwc: out")
        if tuple(out.shape) != shape or out.device != x.device:
            raise _hip.HipError("depthwise_conv3x3_nhwc: out must be %s on %s, got %s" % (shape, x.device, tuple(out.shape)))
    if n == 0:
        return out          # an empty tensor has no storage to point at
    _hip.check(lib.frcnn_dwconv3x3_fwd(_ptr(x), _ptr(w_rsc), _ptr(scale), _ptr(shift), _ptr(out), n, h, w, c, stride,
                                       float(in_cap), float(out_cap), int(bool(relu)), _stream()), "frcnn_dwconv3x3_fwd")
    return out


def clamp_max_(x, cap):
    """x = min(x, cap) in place (frcnn_clamp_max): the upper half of a ReLU6 behind a convolution's ReLU epilogue."""
    lib = _hip.load()
    _dev_f32(x, "clamp_max_: x")
    _hip.check(lib.frcnn_clamp_max(_ptr(x), x.numel(), float(cap), _stream()), "frcnn_clamp_max")
    return x


def _dw_bwd_operands(who, dy, y, scale, x_shape, stride, relu, out_cap):
    """Argument checks shared by the two depthwise gradients: dy (and y, scale) against the INPUT shape (N,H,W,C)."""
    _dev_f32(dy, who + ": dy")
    if len(x_shape) != 4:
        raise _hip.HipError("%s: x must be (N,H,W,C), got %s" % (who, tuple(x_shape)))
    n, h, w, c = (int(v) for v in x_shape)
    stride = int(stride)
    if stride not in (1, 2):
        raise _hip.HipError("%s: stride %d (1 or 2)" % (who, stride))
    shape = (n, (h - 1) // stride + 1, (w - 1) // stride + 1, c)
    if tuple(dy.shape) != shape:
        raise _hip.HipError("%s: dy must be %s for x %s at stride %d, got %s" % (who, shape, (n, h, w, c), stride, tuple(dy.shape)))
    if y is not None:
        _dev_f32(y, who + ": y")
        if tuple(y.shape) != shape or y.device != dy.device:
            raise _hip.HipError("%s: y must be %s on %s, got %s" % (who, shape, dy.device, tuple(y.shape)))
    elif relu or float(out_cap) != float('inf'):
        raise _hip.HipError("%s: y is needed for the mask of relu / out_cap" % who)
    if scale is not None:
        _dev_f32(scale, who + ": scale")
        if tuple(scale.shape) != (c,) or scale.device != dy.device:
            raise _hip.HipError("%s: scale must be (%d,) on %s, got %s" % (who, c, dy.device, tuple(scale.shape)))
    return n, h, w, c, stride


def depthwise_conv3x3_bwd_data(dy, y, w_rsc, x_shape, scale=None, stride=1, relu=False, out_cap=float('inf'), out=None):
    """Data gradient of ``depthwise_conv3x3_nhwc`` (frcnn_dwconv3x3_bwd_data; lib/nets/mobilenet_v1.py:117-123 under
    loss.backward()): dy, y (N,OH,OW,C) - y the forward's stored output, None when neither relu nor out_cap masks -,
    w_rsc (3,3,C) -> the gradient (N,H,W,C) with respect to min(x, in_cap).  ``out``: a tensor of that shape to write into."""
    lib = _hip.load()
    who = "depthwise_conv3x3_bwd_data"
    n, h, w, c, stride = _dw_bwd_operands(who, dy, y, scale, x_shape, stride, relu, out_cap)
    _dev_f32(w_rsc, who + ": w_rsc")
    if tuple(w_rsc.shape) != (3, 3, c) or w_rsc.device != dy.device:
        raise _hip.HipError("%s: w_rsc must be (3,3,%d) on %s, got %s" % (who, c, dy.device, tuple(w_rsc.shape)))
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=dy.device)
    else:
        _dev_f32(out, who + ": out")
        if tuple(out.shape) != (n, h, w, c) or out.device != dy.device:
            raise _hip.HipError("%s: out must be %s on %s, got %s" % (who, (n, h, w, c), dy.device, tuple(out.shape)))
    if n == 0:
        return out
    _hip.check(lib.frcnn_dwconv3x3_bwd_data(_ptr(dy), _ptr(y), _ptr(w_rsc), _ptr(scale), _ptr(out), n, h, w, c, stride,
                                            float(out_cap), int(bool(relu)), _stream()), "frcnn_dwconv3x3_bwd_data")
    return out


def depthwise_conv3x3_bwd_weight(x, dy, y, scale=None, stride=1, relu=False, in_cap=float('inf'), out_cap=float('inf'),
                                 out=None, accumulate=False):
    """Filter gradient of ``depthwise_conv3x3_nhwc`` in the parameter's own (C,1,3,3) layout (frcnn_dwconv3x3_bwd_weight):
    x (N,H,W,C) the forward's input, dy / y (N,OH,OW,C).  ``out``: the buffer to write; ``accumulate``: add into it (a
    parameter's ``.grad``) instead of overwriting.  Deterministic: two calls on the same operands are bit-equal."""
    lib = _hip.load()
    who = "depthwise_conv3x3_bwd_weight"
    _dev_f32(x, who + ": x")
    n, h, w, c, stride = _dw_bwd_operands(who, dy, y, scale, tuple(x.shape), stride, relu, out_cap)
    if x.device != dy.device:
        raise _hip.HipError("%s: x on %s, dy on %s" % (who, x.device, dy.device))
    if out is None:
        if accumulate:
            raise _hip.HipError("%s: accumulate needs out=" % who)
        out = torch.empty((c, 1, 3, 3), dtype=torch.float32, device=x.device)
    else:
        _dev_f32(out, who + ": out")
        if tuple(out.shape) != (c, 1, 3, 3) or out.device != x.device:
            raise _hip.HipError("%s: out must be (%d,1,3,3) on %s, got %s" % (who, c, x.device, tuple(out.shape)))
    if n == 0:              # an empty tensor has no storage to point at: the sum over no pixels
        return out if accumulate else out.zero_()
    ws_bytes = lib.frcnn_dwconv3x3_bwd_weight_ws_bytes(n, h, w, c, stride)
    ws = _workspace(ws_bytes, x.device)
    _hip.check(lib.frcnn_dwconv3x3_bwd_weight(_ptr(x), _ptr(dy), _ptr(y), _ptr(scale), _ptr(out), n, h, w, c, stride,
                                              float(in_cap), float(out_cap), int(bool(relu)), int(bool(accumulate)), _ptr(ws),
                                              ws_bytes, _stream()), "frcnn_dwconv3x3_bwd_weight")
    return out


def act_bwd_cap(dy, y, scale=None, relu=True, cap=float('inf'), out=None):
    """Backward of a ReLU6 behind a GEMM convolution (frcnn_act_bwd_cap): dy * scale[k] * [y > 0 if relu] * [y < cap],
    k = dy.shape[-1]; ``y`` is the convolution's stored output, with or without the upper clamp applied."""
    lib = _hip.load()
    _dev_f32(dy, "act_bwd_cap: dy")
    k = dy.shape[-1] if dy.dim() else 1
    masked = bool(relu) or float(cap) != float('inf')
    if masked or y is not None:
        _dev_f32(y, "act_bwd_cap: y")
        if tuple(y.shape) != tuple(dy.shape) or y.device != dy.device:
            raise _hip.HipError("act_bwd_cap: y must be %s on %s, got %s" % (tuple(dy.shape), dy.device, tuple(y.shape)))
    if scale is not None:
        _dev_f32(scale, "act_bwd_cap: scale")
        if tuple(scale.shape) != (k,) or scale.device != dy.device:
            raise _hip.HipError("act_bwd_cap: scale must be (%d,) on %s, got %s" % (k, dy.device, tuple(scale.shape)))
    if out is None:
        out = torch.empty_like(dy)
    else:
        _dev_f32(out, "act_bwd_cap: out")
        if tuple(out.shape) != tuple(dy.shape) or out.device != dy.device:
            raise _hip.HipError("act_bwd_cap: out must be %s on %s, got %s" % (tuple(dy.shape), dy.device, tuple(out.shape)))
    if dy.numel() == 0:
        return out
    _hip.check(lib.frcnn_act_bwd_cap(_ptr(dy), _ptr(y), _ptr(scale), int(bool(relu)), float(cap), dy.numel() // k, k, _ptr(out),
                                     _stream()), "frcnn_act_bwd_cap")
    return out


def pad_channels(x, c_pad):
    """(N,H,W,C) -> (N,H,W,c_pad) zero-padded channels."""
    lib = _hip.load()
    _dev_f32(x, "x")
    n, h, w, c = x.shape
    if c == c_pad:
        return x
    out = torch.empty((n, h, w, c_pad), dtype=torch.float32, device=x.device)
    _hip.check(lib.frcnn_pad_channels(_ptr(x), _ptr(out), n * h * w, c, c_pad, _stream()), "frcnn_pad_channels")
    return out


def generate_anchors(base_f64, height, width, feat_stride):
    """base_f64: (A,4) float64 DEVICE tensor -> (H*W*A, 4) float32 anchors."""
    lib = _hip.load()
    if not base_f64.is_cuda or base_f64.dtype != torch.float64 or not base_f64.is_contiguous():
        raise _hip.HipError("generate_anchors: base must be a contiguous float64 device tensor")
    a = base_f64.shape[0]
    out = torch.empty((height * width * a, 4), dtype=torch.float32, device=base_f64.device)
    _hip.check(lib.frcnn_generate_anchors(_ptr(base_f64), a, height, width, feat_stride, _ptr(out), _stream()),
               "frcnn_generate_anchors")
    return out


def rpn_decode_clip(anchors, info, num_anchors, rpn=None, probs=None, deltas=None):
    """Front half of proposal_layer. Either `rpn` (H*W, >=6A) fused head output or (probs, deltas).
    info: host sequence [x_min, x_max, y_min, y_max, ...]. Returns (scores (N,), proposals (N,4))."""
    lib = _hip.load()
    _dev_f32(anchors, "anchors")
    total = anchors.shape[0]
    hw = total // num_anchors
    ld = 0
    if rpn is not None:
        _dev_f32(rpn, "rpn")
        ld = rpn.shape[-1]
        if rpn.numel() != hw * ld:
            raise _hip.HipError("rpn_decode_clip: rpn has %d elements, expected %d x %d" % (rpn.numel(), hw, ld))
    if probs is not None:
        _dev_f32(probs, "probs")
        if probs.numel() != total:
            raise _hip.HipError("rpn_decode_clip: probs has %d elements, expected %d" % (probs.numel(), total))
    if deltas is not None:
        _dev_f32(deltas, "deltas")
        if deltas.numel() != total * 4:
            raise _hip.HipError("rpn_decode_clip: deltas has %d elements, expected %d" % (deltas.numel(), total * 4))
    scores = torch.empty((total,), dtype=torch.float32, device=anchors.device)
    props = torch.empty((total, 4), dtype=torch.float32, device=anchors.device)
    info_arr = _hip.float_array([float(v) for v in info[:4]])
    _hip.check(lib.frcnn_rpn_decode_clip(_ptr(rpn), ld, _ptr(probs), _ptr(deltas), _ptr(anchors), info_arr, hw,
                                         num_anchors, _ptr(scores), _ptr(props), _stream()), "frcnn_rpn_decode_clip")
    return scores, props


def bbox_transform_inv(boxes, deltas, scale=None):
    """boxes (N, >=4) [x1,y1,x2,y2,...], deltas (N, 4K) -> (N, 4K) decoded boxes."""
    lib = _hip.load()
    _dev_f32(boxes, "boxes"); _dev_f32(deltas, "deltas")
    n = boxes.shape[0]
    if n == 0:
        return deltas.detach() * 0  # reference: bbox_transform.py:79-80
    k = deltas.shape[1] // 4
    out = torch.empty((n, 4 * k), dtype=torch.float32, device=boxes.device)
    _hip.check(lib.frcnn_bbox_transform_inv(_ptr(boxes), boxes.shape[1], _ptr(deltas), n, k,
                                            float(scale) if scale is not None else 0.0, _ptr(out), _stream()),
               "frcnn_bbox_transform_inv")
    return out


def lidar_bbox_transform_inv(rois, anchors_3d, deltas, scale=None):
    """rois (N, >=4) [x1,y1,x2,y2,...], anchors_3d (N,7), deltas (N,7K) -> (N,7K) [xc,yc,zc,l,w,h,ry] per class."""
    lib = _hip.load()
    _dev_f32(rois, "rois"); _dev_f32(anchors_3d, "anchors_3d"); _dev_f32(deltas, "deltas")
    n = rois.shape[0]
    if n == 0:
        return deltas.detach() * 0  # reference: bbox_transform.py:181-182
    k = deltas.shape[1] // 7
    out = torch.empty((n, 7 * k), dtype=torch.float32, device=rois.device)
    _hip.check(lib.frcnn_lidar_bbox_transform_inv(_ptr(rois), rois.shape[1], _ptr(anchors_3d), _ptr(deltas), n, k,
                                                  float(scale) if scale is not None else 0.0, _ptr(out), _stream()),
               "frcnn_lidar_bbox_transform_inv")
    return out


def uncertainty_transform_inv(rois, uncertainty, anchors_3d=None, scale=None, lidar=False, input_is_variance=False):
    """uncertainty (N, 7K) of the 7-element deltas -> squared box-space terms: (N, 4K) [x,y,l,w] (lidar False) or (N, 7K)."""
    lib = _hip.load()
    _dev_f32(rois, "rois"); _dev_f32(uncertainty, "uncertainty")
    n = rois.shape[0]
    if uncertainty.shape[0] != n or uncertainty.shape[1] % 7:
        raise _hip.HipError("uncertainty_transform_inv: uncertainty must be (N, 7K), got %s" % (tuple(uncertainty.shape),))
    k = uncertainty.shape[1] // 7
    out = torch.empty((n, (7 if lidar else 4) * k), dtype=torch.float32, device=rois.device)
    if lidar:
        _dev_f32(anchors_3d, "anchors_3d")
    if n:
        _hip.check(lib.frcnn_uncertainty_transform_inv(_ptr(rois), rois.shape[1], _ptr(anchors_3d) if lidar else None,
                                                       _ptr(uncertainty), n, k, float(scale) if scale is not None else 0.0,
                                                       1 if lidar else 0, 1 if input_is_variance else 0, _ptr(out), _stream()),
                   "frcnn_uncertainty_transform_inv")
    return out


def clip_boxes(boxes, info):
    lib = _hip.load()
    _dev_f32(boxes, "boxes")
    out = torch.empty_like(boxes)
    if boxes.numel() == 0:
        return out
    _hip.check(lib.frcnn_clip_boxes(_ptr(boxes), boxes.numel() // 4, _hip.float_array([float(v) for v in info[:4]]),
                                    _ptr(out), _stream()), "frcnn_clip_boxes")
    return out


def sort_topk_desc(scores, top_n):
    """Returns (order int64 (top_n,), sorted_scores (top_n,), count int32 (1,)) — (score desc, index asc)."""
    lib = _hip.load()
    _dev_f32(scores, "scores")
    n = scores.numel()
    m = min(n, top_n)
    order = torch.empty((m,), dtype=torch.int64, device=scores.device)
    sout = torch.empty((m,), dtype=torch.float32, device=scores.device)
    count = torch.empty((1,), dtype=torch.int32, device=scores.device)
    ws_bytes = lib.frcnn_sort_topk_desc_ws_bytes(n, top_n)
    ws = _workspace(ws_bytes, scores.device) if ws_bytes else None
    _hip.check(lib.frcnn_sort_topk_desc(_ptr(scores), n, top_n, _ptr(order), _ptr(sout), _ptr(count), _ptr(ws), ws_bytes,
                                        _stream()), "frcnn_sort_topk_desc")
    return order, sout, count


def gather_rows(rows, order, count=None):
    lib = _hip.load()
    _dev_f32(rows, "rows")
    width = rows.shape[1] if rows.dim() > 1 else 1
    m = order.numel()
    out = torch.empty((m, width), dtype=torch.float32, device=rows.device)
    _hip.check(lib.frcnn_gather_rows(_ptr(rows), _ptr(order), _ptr(count), m, width, _ptr(out), _stream()),
               "frcnn_gather_rows")
    return out


def uncertainty_columns(dets, det_roi, sources, out=None):
    """Detections followed by their uncertainty columns in ONE launch (nms_hstack_var_torch, filter_predictions.py:23-43,
    and the stacking of lib/model/test.py:260-270).  dets (K, M, D) float32, det_roi (K, M) int32 RoI row of each
    detection (-1 = padding), ``sources`` a sequence of up to 8 ``(tensor, per_class)``: a per-class source is
    (R, K * w) and class j takes columns [j*w, (j+1)*w) of its RoI's row; a shared source is (R, w) or (R,) and every
    class takes the whole row.  Returns (K, M, D + U); padding rows keep their box columns and get +0.0 after them."""
    lib = _hip.load()
    _dev_f32(dets, "dets")
    if dets.dim() != 3 or det_roi.dtype != torch.int32 or not det_roi.is_cuda or not det_roi.is_contiguous() or \
            tuple(det_roi.shape) != tuple(dets.shape[:2]):
        raise _hip.HipError("uncertainty_columns: dets (K, M, D) float32 and det_roi (K, M) int32, contiguous, on the device")
    k, m, d = dets.shape
    if not sources or len(sources) > 8:
        raise _hip.HipError("uncertainty_columns: 1 to 8 sources, got %d" % len(sources))
    r = sources[0][0].shape[0]
    ptrs, widths, kinds = [], [], []
    for i, (v, per_class) in enumerate(sources):
        _dev_f32(v, "source %d" % i)
        cols = v.shape[1] if v.dim() == 2 else 1
        if v.dim() not in (1, 2) or v.shape[0] != r or (per_class and (v.dim() != 2 or cols % k)):
            raise _hip.HipError("uncertainty_columns: source %d is %s for %d RoIs and %d classes" % (i, tuple(v.shape), r, k))
        ptrs.append(v.data_ptr()); widths.append(cols // k if per_class else cols); kinds.append(1 if per_class else 0)
    w = d + sum(widths)
    if out is None:
        out = torch.empty((k, m, w), dtype=torch.float32, device=dets.device)
    elif tuple(out.shape) != (k, m, w) or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise _hip.HipError("uncertainty_columns: out must be a contiguous float32 (%d, %d, %d) device tensor" % (k, m, w))
    if k * m == 0:
        return out
    ns = len(ptrs)
    _hip.check(lib.frcnn_uncertainty_columns(_ptr(dets), _ptr(det_roi), k, m, d, r, ns, (ctypes.c_void_p * ns)(*ptrs),
                                             (ctypes.c_int * ns)(*widths), (ctypes.c_int * ns)(*kinds), _ptr(out), _stream()),
               "frcnn_uncertainty_columns")
    return out


def set_nms_suppress_at_equal(on):
    """IoU == threshold exactly: True (default) suppresses like torchvision 0.4.0's CPU kernel (`>=`), False keeps the box
    like its CUDA kernel (`>`).  Returns the previous setting."""
    lib = _hip.load()
    old = bool(lib.frcnn_nms_get_suppress_at_equal())
    _hip.check(lib.frcnn_nms_set_suppress_at_equal(1 if on else 0), "frcnn_nms_set_suppress_at_equal")
    return old


def nms_suppress_at_equal():
    """The current rule at IoU == threshold exactly (frcnn_nms_get_suppress_at_equal).  The rule is read at LAUNCH time, so
    a captured frame keeps the rule of its capture: model/frame_graph.cfg_fingerprint keys the captured frames by it."""
    return bool(_hip.load().frcnn_nms_get_suppress_at_equal())


def nms_sorted(boxes, thresh, max_keep=None, n_dev=None, want_mask=False):
    """NMS over boxes already in descending-score order.
    Returns (keep_idx int64 (max_keep,), keep_count int32 (1,), keep_mask uint8 (n,) or None)."""
    lib = _hip.load()
    _dev_f32(boxes, "boxes")
    n = boxes.shape[0]
    max_keep = n if max_keep is None or max_keep <= 0 else min(max_keep, n)
    keep_idx = torch.empty((max_keep,), dtype=torch.int64, device=boxes.device)     # the kernel zeroes the unused tail
    keep_count = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    keep_mask = torch.empty((n,), dtype=torch.uint8, device=boxes.device) if want_mask else None
    ws_bytes = lib.frcnn_nms_ws_bytes(n)
    ws = _workspace(ws_bytes, boxes.device)
    _hip.check(lib.frcnn_nms(_ptr(boxes), _ptr(n_dev), n, float(thresh), max_keep, _ptr(keep_idx), _ptr(keep_mask),
                             _ptr(keep_count), _ptr(ws), ws_bytes, _stream()), "frcnn_nms")
    return keep_idx, keep_count, keep_mask


def nms_rotated(boxes, thresh, n=None, max_keep=None):
    """Rotated BEV NMS over 7-DoF boxes (n_max, 7) [xc,yc,zc,l,w,h,ry] already in descending-score order
    (frcnn_nms_rotated; the float64 rule of utils/bbox.nms_rotated_host).  ``n``: device int32 tensor holding the live count
    (None: every row).  Returns (keep_idx int64 (max_keep,), keep_count int32 (1,)); entries past the count are 0."""
    lib = _hip.load()
    _dev_f32(boxes, "boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 7 or boxes.shape[0] == 0:
        raise _hip.HipError("nms_rotated: boxes must be (N>0, 7), got %s" % (tuple(boxes.shape),))
    if n is not None and not (isinstance(n, torch.Tensor) and n.is_cuda and n.dtype == torch.int32):
        raise _hip.HipError("nms_rotated: n must be a device int32 tensor (the live count is read on the device)")
    n_max = boxes.shape[0]
    max_keep = n_max if max_keep is None or max_keep <= 0 else min(int(max_keep), n_max)
    keep_idx = torch.empty((max_keep,), dtype=torch.int64, device=boxes.device)     # the kernel zeroes the unused tail
    keep_count = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    ws_bytes = lib.frcnn_nms_rotated_ws_bytes(n_max)
    ws = _workspace(ws_bytes, boxes.device)
    _hip.check(lib.frcnn_nms_rotated(_ptr(boxes), _ptr(n), n_max, float(thresh), max_keep, _ptr(keep_idx), None,
                                     _ptr(keep_count), _ptr(ws), ws_bytes, _stream()), "frcnn_nms_rotated")
    return keep_idx, keep_count


def make_rois(sorted_boxes, sorted_scores, keep_idx, keep_count):
    lib = _hip.load()
    m = keep_idx.numel()
    rois = torch.empty((m, 5), dtype=torch.float32, device=sorted_boxes.device)
    roi_scores = torch.empty((m, 1), dtype=torch.float32, device=sorted_boxes.device)
    _hip.check(lib.frcnn_make_rois(_ptr(sorted_boxes), _ptr(sorted_scores), _ptr(keep_idx), _ptr(keep_count), m,
                                   _ptr(rois), _ptr(roi_scores), _stream()), "frcnn_make_rois")
    return rois, roi_scores


def _roi_epilogue_and_plan(who, lib, feat, r, pooled, plan_c, scale, shift):
    """What the RoIAlign forwards share: checks the optional per-channel ``scale`` / ``shift`` against feat's channels and
    returns the plan workspace ``(ws, ws_bytes)`` of a map with ``plan_c`` channels; ws is None when pooled has no plan."""
    _, h, w, c = feat.shape
    for nm, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _dev_f32(t, nm)
            if t.numel() != c:
                raise _hip.HipError("%s: %s has %d elements, expected %d" % (who, nm, t.numel(), c))
    ws_bytes = lib.frcnn_roi_align_fwd_ws_bytes(h, w, plan_c, r, pooled)
    return (_workspace(ws_bytes, feat.device) if ws_bytes else None), ws_bytes


def roi_align_nhwc(feat, rois, pooled, spatial_scale, sampling_ratio=0, roi_count=None, level_of_roi=None, level=-1,
                   out=None, rois_per_image=0, scale=None, shift=None, relu=False):
    """feat (N,H,W,C), rois (R,5) -> (R, P, P, C).  ``rois_per_image`` > 0: rows [i*rpi, (i+1)*rpi) belong to image i and
    ``roi_count`` holds N live counts (frames batched into one call); 0: the image is the RoI's batch column.
    ``scale`` / ``shift`` (C,) / ``relu``: per-channel epilogue on the pooled values, out = act(pooled * scale + shift)
    (frcnn_roi_align_fwd_affine; without them it is what frcnn_roi_align_fwd computes)."""
    lib = _hip.load()
    _dev_f32(feat, "feat"); _dev_f32(rois, "rois")
    n, h, w, c = feat.shape
    r = rois.shape[0]
    ws, ws_bytes = _roi_epilogue_and_plan("roi_align_nhwc", lib, feat, r, pooled, c, scale, shift)
    if out is None:
        out = torch.empty((r, pooled, pooled, c), dtype=torch.float32, device=feat.device)
    _hip.check(lib.frcnn_roi_align_fwd_affine(_ptr(feat), n, h, w, c, _ptr(rois), _ptr(roi_count), r, int(rois_per_image),
                                              pooled, float(spatial_scale), int(sampling_ratio), _ptr(level_of_roi), level,
                                              _ptr(out), _ptr(scale), _ptr(shift), int(bool(relu)), _ptr(ws), ws_bytes,
                                              _stream()), "frcnn_roi_align_fwd_affine")
    return out


def roi_align_split(feat, rois, pooled, spatial_scale, split_c, sampling_ratio=0, roi_count=None, scale=None, shift=None,
                    relu1=False, relu2=False):
    """(out1 (R,P,P,split_c), out2 (R,P,P,C - split_c)) = RoIAlign of feat (1,H,W,C) over the two channel ranges with one
    plan (frcnn_roi_align_fwd_split); ``scale`` / ``shift`` (C,) are applied after the pooling, ReLU per output."""
    lib = _hip.load()
    _dev_f32(feat, "feat"); _dev_f32(rois, "rois")
    n, h, w, c = feat.shape
    if n != 1 or rois.shape[1] != 5:
        raise _hip.HipError("roi_align_split: one image, rois (R,5)")
    r = rois.shape[0]
    ws, ws_bytes = _roi_epilogue_and_plan("roi_align_split", lib, feat, r, pooled, 4, scale, shift)   # one descriptor per piece
    out1 = torch.empty((r, pooled, pooled, split_c), dtype=torch.float32, device=feat.device)
    out2 = torch.empty((r, pooled, pooled, c - split_c), dtype=torch.float32, device=feat.device)
    _hip.check(lib.frcnn_roi_align_fwd_split(_ptr(feat), h, w, c, _ptr(rois), _ptr(roi_count), r, pooled, float(spatial_scale),
                                             int(sampling_ratio), int(split_c), _ptr(out1), _ptr(out2), _ptr(scale), _ptr(shift),
                                             int(bool(relu1)), int(bool(relu2)), _ptr(ws), ws_bytes, _stream()),
               "frcnn_roi_align_fwd_split")
    return out1, out2


def head_fc_softmax_decode(x, w_cls, b_cls, w_box, b_box, rois, stds, means, scale, roi_anchors_3d=None):
    """x (R,P,P,C) -> dict(fc7, cls_score, cls_prob, bbox_pred, pred_boxes).  With ``roi_anchors_3d`` (R,7) the
    boxes are the 7-DoF LiDAR boxes (frcnn_head_fc_softmax_decode_lidar), otherwise 4-DoF image boxes."""
    lib = _hip.load()
    for nm, t in (("x", x), ("w_cls", w_cls), ("b_cls", b_cls), ("w_box", w_box), ("b_box", b_box), ("rois", rois)):
        _dev_f32(t, nm)
    r, p, _, c = x.shape
    k = w_cls.shape[0]
    e = 4 if roi_anchors_3d is None else 7
    if w_box.shape[0] != e * k or w_cls.shape[1] != c or w_box.shape[1] != c or len(stds) != e or len(means) != e:
        raise _hip.HipError("head_fc_softmax_decode: inconsistent head weights / normalisation for %d-DoF boxes" % e)
    dev = x.device
    fc7 = torch.empty((r, c), dtype=torch.float32, device=dev)
    cls_score = torch.empty((r, k), dtype=torch.float32, device=dev)
    cls_prob = torch.empty((r, k), dtype=torch.float32, device=dev)
    bbox_pred = torch.empty((r, e * k), dtype=torch.float32, device=dev)
    pred_boxes = torch.empty((r, e * k), dtype=torch.float32, device=dev)
    if e == 4:
        _hip.check(lib.frcnn_head_fc_softmax_decode(
            _ptr(x), r, p, c, _ptr(w_cls), _ptr(b_cls), _ptr(w_box), _ptr(b_box), k, _ptr(rois),
            _hip.float_array(stds), _hip.float_array(means), float(scale), _ptr(fc7), _ptr(cls_score), _ptr(cls_prob),
            _ptr(bbox_pred), _ptr(pred_boxes), _stream()), "frcnn_head_fc_softmax_decode")
    else:
        _dev_f32(roi_anchors_3d, "roi_anchors_3d")
        if tuple(roi_anchors_3d.shape) != (r, 7):
            raise _hip.HipError("head_fc_softmax_decode: roi_anchors_3d must be (%d, 7)" % r)
        _hip.check(lib.frcnn_head_fc_softmax_decode_lidar(
            _ptr(x), r, p, c, _ptr(w_cls), _ptr(b_cls), _ptr(w_box), _ptr(b_box), k, _ptr(rois), _ptr(roi_anchors_3d),
            _hip.float_array(stds), _hip.float_array(means), float(scale), _ptr(fc7), _ptr(cls_score), _ptr(cls_prob),
            _ptr(bbox_pred), _ptr(pred_boxes), _stream()), "frcnn_head_fc_softmax_decode_lidar")
    return {"fc7": fc7, "cls_score": cls_score, "cls_prob": cls_prob, "bbox_pred": bbox_pred, "pred_boxes": pred_boxes}


HEAD_FUSED_MAX_OUT = 64          # MAX_OUT of csrc/head.hip: the fused tail keeps a RoI's K + E*K head outputs in LDS


def head_uses_wide_form(num_classes, box_elems):
    """Which form of the detection tail runs a frame: the fused one-workgroup-per-RoI kernel (head_fc_softmax_decode) where it
    accepts the class count, K * (1 + E) <= 64, i.e. up to 12 classes for image boxes (E = 4) and 8 for LiDAR boxes (E = 7);
    the GEMM-tiled wide form (head_softmax_decode_wide) for every larger K."""
    return int(num_classes) * (1 + int(box_elems)) > HEAD_FUSED_MAX_OUT


def head_softmax_decode_wide(fc7, w_cls, b_cls, w_box, b_box, rois, stds, means, scale, roi_anchors_3d=None):
    """fc7 (R,C) -> dict(fc7, cls_score, cls_prob, bbox_pred, pred_boxes) for any class count; ``fc7`` is the input tensor.
    The two heads as one MFMA GEMM, then softmax and decode (frcnn_head_wide_softmax_decode[_lidar]).  With
    ``roi_anchors_3d`` (R,7) the boxes are the 7-DoF LiDAR boxes, otherwise 4-DoF image boxes."""
    lib = _hip.load()
    for nm, t in (("fc7", fc7), ("w_cls", w_cls), ("b_cls", b_cls), ("w_box", w_box), ("b_box", b_box), ("rois", rois)):
        _dev_f32(t, nm)
    if fc7.dim() != 2:
        raise _hip.HipError("head_softmax_decode_wide: fc7 must be (R, C)")
    r, c = fc7.shape
    k = w_cls.shape[0]
    e = 4 if roi_anchors_3d is None else 7
    if (w_box.shape[0] != e * k or w_cls.shape[1] != c or w_box.shape[1] != c or b_cls.numel() != k or b_box.numel() != e * k
            or len(stds) != e or len(means) != e or tuple(rois.shape) != (r, 5)):
        raise _hip.HipError("head_softmax_decode_wide: inconsistent head weights / rois / normalisation for %d-DoF boxes" % e)
    dev = fc7.device
    cls_score = torch.empty((r, k), dtype=torch.float32, device=dev)
    cls_prob = torch.empty((r, k), dtype=torch.float32, device=dev)
    bbox_pred = torch.empty((r, e * k), dtype=torch.float32, device=dev)
    pred_boxes = torch.empty((r, e * k), dtype=torch.float32, device=dev)
    if e == 4:
        _hip.check(lib.frcnn_head_wide_softmax_decode(
            _ptr(fc7), r, c, _ptr(w_cls), _ptr(b_cls), _ptr(w_box), _ptr(b_box), k, _ptr(rois),
            _hip.float_array(stds), _hip.float_array(means), float(scale), _ptr(cls_score), _ptr(cls_prob),
            _ptr(bbox_pred), _ptr(pred_boxes), _stream()), "frcnn_head_wide_softmax_decode")
    else:
        _dev_f32(roi_anchors_3d, "roi_anchors_3d")
        if tuple(roi_anchors_3d.shape) != (r, 7):
            raise _hip.HipError("head_softmax_decode_wide: roi_anchors_3d must be (%d, 7)" % r)
        _hip.check(lib.frcnn_head_wide_softmax_decode_lidar(
            _ptr(fc7), r, c, _ptr(w_cls), _ptr(b_cls), _ptr(w_box), _ptr(b_box), k, _ptr(rois), _ptr(roi_anchors_3d),
            _hip.float_array(stds), _hip.float_array(means), float(scale), _ptr(cls_score), _ptr(cls_prob),
            _ptr(bbox_pred), _ptr(pred_boxes), _stream()), "frcnn_head_wide_softmax_decode_lidar")
    return {"fc7": fc7, "cls_score": cls_score, "cls_prob": cls_prob, "bbox_pred": bbox_pred, "pred_boxes": pred_boxes}


def generate_anchors_3d(base, height, width, feat_stride):
    """base: DEVICE float32 (T, 9) anchor-type table -> (anchors_3d (H*W*T, 7), anchors_2d (H*W*T, 4))."""
    lib = _hip.load()
    _dev_f32(base, "base")
    t = base.shape[0]
    a3 = torch.empty((height * width * t, 7), dtype=torch.float32, device=base.device)
    a2 = torch.empty((height * width * t, 4), dtype=torch.float32, device=base.device)
    _hip.check(lib.frcnn_generate_anchors_3d(_ptr(base), t, height, width, feat_stride, _ptr(a3), _ptr(a2), _stream()),
               "frcnn_generate_anchors_3d")
    return a3, a2


def filter_per_class_lidar(pred_boxes, cls_prob, thresh, nms_thresh, max_dets, max_out=None, roi_count=None,
                           want_rois=False, rotated=False):
    """7-DoF form: returns (dets (K, max_out, 8) [xc,yc,zc,l,w,h,ry,score], det_count int32 (K,)[, det_roi int32
    (K, max_out)]).  ``rotated``: suppress on the rotated BEV footprints (frcnn_filter_per_class_lidar_rot, the rule of
    utils/bbox.nms_rotated_host) instead of the reference's yaw-less rectangles; same outputs, same shapes."""
    lib = _hip.load()
    _dev_f32(pred_boxes, "pred_boxes"); _dev_f32(cls_prob, "cls_prob")
    r, k = cls_prob.shape
    if pred_boxes.shape[1] != 7 * k:
        raise _hip.HipError("filter_per_class_lidar: pred_boxes must be (R, 7K)")
    max_out = r if max_out is None else max_out
    dets = torch.empty((k, max_out, 8), dtype=torch.float32, device=cls_prob.device)    # every row is written by the call
    det_count = torch.empty((k,), dtype=torch.int32, device=cls_prob.device)
    name = "frcnn_filter_per_class_lidar_rot" if rotated else "frcnn_filter_per_class_lidar"
    ws_bytes = (lib.frcnn_filter_per_class_lidar_rot_ws_bytes if rotated else lib.frcnn_filter_per_class_ws_bytes)(r, k)
    ws = _workspace(ws_bytes, cls_prob.device)
    det_roi = torch.empty((k, max_out), dtype=torch.int32, device=cls_prob.device) if want_rois else None   # -1 = no detection
    _hip.check(getattr(lib, name)(_ptr(pred_boxes), _ptr(cls_prob), _ptr(roi_count), r, k, float(thresh),
                                  float(nms_thresh), int(max_dets), int(max_out), _ptr(dets), _ptr(det_count),
                                  _ptr(det_roi), _ptr(ws), ws_bytes, _stream()), name)
    return (dets, det_count, det_roi) if want_rois else (dets, det_count)


def filter_per_class(pred_boxes, cls_prob, frame_w, frame_h, scale, thresh, nms_thresh, max_dets, max_out=None,
                     roi_count=None, want_rois=False):
    """In-place clamp of pred_boxes + per-class threshold/NMS/max_dets.
    Returns (dets (K, max_out, 5), det_count int32 (K,)[, det_roi int32 (K, max_out): RoI row of each detection])."""
    lib = _hip.load()
    _dev_f32(pred_boxes, "pred_boxes"); _dev_f32(cls_prob, "cls_prob")
    r, k = cls_prob.shape
    max_out = r if max_out is None else max_out
    dets = torch.empty((k, max_out, 5), dtype=torch.float32, device=cls_prob.device)    # every row is written by the call
    det_count = torch.empty((k,), dtype=torch.int32, device=cls_prob.device)
    ws_bytes = lib.frcnn_filter_per_class_ws_bytes(r, k)
    ws = _workspace(ws_bytes, cls_prob.device)
    det_roi = torch.empty((k, max_out), dtype=torch.int32, device=cls_prob.device) if want_rois else None   # -1 = no detection
    _hip.check(lib.frcnn_filter_per_class(_ptr(pred_boxes), _ptr(cls_prob), _ptr(roi_count), r, k, float(frame_w),
                                          float(frame_h), float(scale), float(thresh), float(nms_thresh), int(max_dets),
                                          int(max_out), _ptr(dets), _ptr(det_count), _ptr(det_roi), _ptr(ws), ws_bytes,
                                          _stream()), "frcnn_filter_per_class")
    return (dets, det_count, det_roi) if want_rois else (dets, det_count)


def bev_voxelize(points, pc_range, voxel_size, z_shift, max_points, max_voxels, num_slices, num_meta,
                 elongation_col=-1):
    """Point cloud (N, F>=4) device tensor -> BEV map (gy, gx, num_slices+num_meta) and the device count of occupied
    cells (frcnn_bev_voxelize_h; lib/roi_data_layer/minibatch.py:434-512).  voxel_size[2] travels twice: rounded to
    fp32 with the other two for the cells, and as the Python float it is for the height slices' float64 product."""
    lib = _hip.load()
    _dev_f32(points, "points")
    if points.dim() != 2 or points.shape[1] < 4 or points.shape[0] == 0:
        raise _hip.HipError("bev_voxelize: points must be (N>0, F>=4), got %s" % (tuple(points.shape),))
    rng, vs = _hip.float_array(pc_range), _hip.float_array(voxel_size)
    grid = (ctypes.c_int * 3)()
    _hip.check(lib.frcnn_bev_voxelize_grid(rng, vs, grid), "frcnn_bev_voxelize_grid")
    gx, gy = int(grid[0]), int(grid[1])
    bev = torch.empty((gy, gx, int(num_slices) + int(num_meta)), dtype=torch.float32, device=points.device)
    count = torch.zeros((1,), dtype=torch.int32, device=points.device)
    nbytes = lib.frcnn_bev_voxelize_ws_bytes(points.shape[0], rng, vs, int(max_voxels))
    ws = _workspace(nbytes, points.device)
    _hip.check(lib.frcnn_bev_voxelize_h(_ptr(points), points.shape[0], points.shape[1], rng, vs, float(voxel_size[2]),
                                        float(z_shift), int(max_points), int(max_voxels), int(num_slices), int(num_meta),
                                        int(elongation_col), _ptr(bev), _ptr(count), _ptr(ws), nbytes, _stream()),
               "frcnn_bev_voxelize_h")
    return bev, count


# frcnn_lidar_augment: flag bits and parameter slots of include/frcnn_hip.h
AUG_GAUSS, AUG_DROPOUT, AUG_ROTATE, AUG_SWAP_XY, AUG_FLIP_Y, AUG_FLIP_X, AUG_RAIN, AUG_TEST_DROPOUT = (1 << b for b in range(8))
# counter-based draws of the kernel (csrc/rng.h): normal01 streams of the distortion (x, y, z) and of the rain shift,
# uniform01 streams of the two keep masks
# frcnn_image_augment: normal01 streams of the additive noise (one per channel), uniform01 stream of the pixel dropout
# frcnn_image_spatter: normal01 stream of the liquid field (reads the uniform streams 88 and 89)
AUG_STREAM = {'gauss_x': 32, 'gauss_y': 33, 'gauss_z': 34, 'rain': 35, 'dropout': 72, 'test_dropout': 73,
              'image_noise_0': 40, 'image_noise_1': 41, 'image_noise_2': 42, 'image_dropout': 86, 'image_spatter': 44}


def _fov_arguments(proj, img_size):
    """(double[12] row-major M, img_h, img_w) of ``proj`` (3x4, anything numpy reads) and ``img_size`` = [height, width]."""
    import numpy as np
    m = np.asarray(proj, dtype=np.float64)
    if m.shape != (3, 4):
        raise _hip.HipError("proj must be a 3x4 matrix (roi_data_layer.lidar_calib), got shape %s" % (m.shape,))
    if img_size is None or len(img_size) != 2:
        raise _hip.HipError("img_size must be [height, width] (cfg.<DB_NAME>.IMG_SIZE), got %r" % (img_size,))
    return (ctypes.c_double * 12)(*[float(v) for v in m.reshape(-1)]), int(img_size[0]), int(img_size[1])


def lidar_augment_points(points, params, seed, pc_extents, seed_dev=None, out=None, max_blocks=0, proj=None, img_size=None):
    """Per-point LiDAR augmentation / rain simulation in front of ``bev_voxelize`` (frcnn_lidar_augment;
    lib/roi_data_layer/minibatch.py:274-428).  ``points`` (N, F>=4) device tensor; ``params``: the decision record
    (``roi_data_layer.lidar_augment.LidarAugment`` or any object with its fields: flip_x, flip_y, gauss (sx, sy, sz) or
    None, p_keep or None, rotation (radians) or None, swap_xy, rain_rate or None, rain_max_range, test_dropout);
    ``pc_extents`` = [X0, Y0, Z0, X1, Y1, Z1].  Returns (points_out, kept_count): dropped rows carry NaN in x, y, z,
    kept_count is a one-element int32 device tensor (surviving points inside the extents).  ``out=points`` works in place.
    ``proj`` (3x4 float64, ``roi_data_layer.lidar_calib``) with ``img_size`` = [height, width]: the camera field-of-view
    filter of KITTI / CADC scans (:251-268,678-693) runs as the first step of the same pass (frcnn_lidar_augment_fov)."""
    import math
    if (proj is None) != (img_size is None):
        raise _hip.HipError("lidar_augment_points: proj and img_size go together")
    lib = _hip.load()
    _dev_f32(points, "points")
    if points.dim() != 2 or points.shape[1] < 4 or points.shape[0] == 0:
        raise _hip.HipError("lidar_augment_points: points must be (N>0, F>=4), got %s" % (tuple(points.shape),))
    if out is None:
        out = torch.empty_like(points)
    elif _dev_f32(out, "out").shape != points.shape:
        raise _hip.HipError("lidar_augment_points: out %s != points %s" % (tuple(out.shape), tuple(points.shape)))
    flags, vals = 0, [0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    if params.gauss is not None:
        flags |= AUG_GAUSS
        vals[0:3] = [float(v) for v in params.gauss]
    if params.p_keep is not None:
        flags |= AUG_DROPOUT
        vals[3] = float(params.p_keep)
    if params.rotation is not None:
        flags |= AUG_ROTATE
        vals[4], vals[5] = math.cos(float(params.rotation)), math.sin(float(params.rotation))
    if params.rain_rate is not None:
        flags |= AUG_RAIN
        vals[6], vals[7] = float(params.rain_rate), float(params.rain_max_range)
    flags |= (AUG_SWAP_XY if params.swap_xy else 0) | (AUG_FLIP_Y if params.flip_y else 0)
    flags |= (AUG_FLIP_X if params.flip_x else 0) | (AUG_TEST_DROPOUT if params.test_dropout else 0)
    kept = torch.empty((1,), dtype=torch.int32, device=points.device)
    if proj is not None:
        m, img_h, img_w = _fov_arguments(proj, img_size)
        _hip.check(lib.frcnn_lidar_augment_fov(_ptr(points), points.shape[0], points.shape[1], _hip.float_array(pc_extents),
                                               flags, _hip.float_array(vals), int(seed) & 0xFFFFFFFF, _seed_dev(seed_dev),
                                               _ptr(out), _ptr(kept), int(max_blocks), m, img_h, img_w, _stream()),
                   "frcnn_lidar_augment_fov")
        return out, kept
    _hip.check(lib.frcnn_lidar_augment(_ptr(points), points.shape[0], points.shape[1], _hip.float_array(pc_extents), flags,
                                       _hip.float_array(vals), int(seed) & 0xFFFFFFFF, _seed_dev(seed_dev), _ptr(out),
                                       _ptr(kept), int(max_blocks), _stream()), "frcnn_lidar_augment")
    return out, kept


class _NoAugmentation:
    """The identity decision record (the fields ``lidar_augment_points`` reads)."""
    flip_x = flip_y = swap_xy = test_dropout = False
    gauss = p_keep = rotation = rain_rate = None
    rain_max_range = 0.0


def lidar_fov_filter(points, proj, img_size, out=None, max_blocks=0):
    """Camera field-of-view filter of a KITTI / CADC scan alone (frcnn_lidar_augment_fov with every other step off and the
    range wide open; lib/roi_data_layer/minibatch.py:251-268,678-693).  ``points`` (N, F>=4) device tensor, ``proj`` the
    3x4 float64 LiDAR -> pixel matrix of ``roi_data_layer.lidar_calib``, ``img_size`` = [height, width].  Returns
    (points_out, kept): rows that project outside the frame carry NaN in x, y, z (columns 3.. untouched), every other row
    is the input row; kept is a one-element int32 device tensor (points inside the frame)."""
    inf = float("inf")
    return lidar_augment_points(points, _NoAugmentation, 0, [-inf, -inf, -inf, inf, inf, inf], out=out,
                                max_blocks=max_blocks, proj=proj, img_size=img_size)


# frcnn_image_augment: stage codes and the parameter slots per stage of include/frcnn_hip.h
(IMG_COPY, IMG_GAUSS, IMG_AVERAGE, IMG_MEDIAN, IMG_SHARPEN, IMG_NOISE, IMG_HUE_SAT, IMG_AFFINE, IMG_DROPOUT) = range(9)
IMG_MAX_STAGES, IMG_NUM_PARAMS = 8, 12


def image_augment_stages(aug, height, width):
    """``(flip, [(code, [parameters]), ...])`` of an ``ImageAugment`` record (or any object with its fields) for a frame
    of ``height`` x ``width``: the host-side numbers of every stage, computed in double and rounded once to float32 by
    the call (Gaussian taps, sharpen weights, the hue offset on the 0..180 circle, the inverse affine matrix).  Stages
    that change nothing (empty filter group, 1x1 average / median) are left out."""
    import numpy as np
    from .roi_data_layer.image_augment import gaussian_taps, hue_offset
    stages = []
    for st in aug.stages:
        kind = st[0]
        if kind == 'gaussian':
            taps = gaussian_taps(st[1])
            stages.append((IMG_GAUSS, [len(taps)] + [float(t) for t in taps]))
        elif kind == 'average':
            if int(st[1]) != 1:
                stages.append((IMG_AVERAGE, [int(st[1])]))
        elif kind == 'median':
            if int(st[1]) != 1:
                stages.append((IMG_MEDIAN, []))
        elif kind == 'sharpen':
            alpha, light = float(st[1]), float(st[2])
            stages.append((IMG_SHARPEN, [(1.0 - alpha) + alpha * (8.0 + light), -alpha]))
        elif kind == 'noise':
            stages.append((IMG_NOISE, [float(st[1])]))
        elif kind == 'hue_sat':
            stages.append((IMG_HUE_SAT, [float(hue_offset(st[1])), float(st[2])]))
        elif kind != 'none':
            raise _hip.HipError("image_augment: unknown stage %r" % (st,))
    if aug.affine is not None:
        inv = np.linalg.inv(aug.affine.matrix(width, height))
        stages.append((IMG_AFFINE, [inv[0, 0], inv[0, 1], inv[0, 2], inv[1, 0], inv[1, 1], inv[1, 2],
                                    float(aug.affine.order), float(aug.affine.cval)]))
    if aug.dropout is not None:
        stages.append((IMG_DROPOUT, [float(aug.dropout[0]), 1.0 if aug.dropout[1] else 0.0]))
    return bool(aug.flip), stages


def image_augment(img, aug, out=None, scratch=None, seed_dev=None, debug_pre=None):
    """Image augmentation in front of ``prep_im_for_blob`` (frcnn_image_augment; lib/roi_data_layer/minibatch.py:540-647).
    ``img``: uint8 (H, W, 3) device tensor in cv2.imread order; ``aug``: the decision record
    (``roi_data_layer.image_augment.ImageAugment``).  Returns the augmented uint8 frame (``out`` or a new tensor).
    ``scratch``: a uint8 device tensor of at least ``frcnn_image_augment_ws_bytes`` bytes (allocated when a second stage
    needs it and none is given).  ``img``, ``out`` and ``scratch`` must be three different buffers.  ``debug_pre``: float32
    (H, W, 3) device tensor receiving the values before rounding of a single noise / hue-saturation stage (tests)."""
    lib = _hip.load()
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise _hip.HipError("image_augment: img must be a tensor on the MI355X (got %s); this package has no CPU path"
                            % (getattr(img, "device", type(img)),))
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous():
        raise _hip.HipError("image_augment: img must be a contiguous uint8 (H, W, 3) frame, got %s %s"
                            % (img.dtype, tuple(img.shape)))
    h, w = int(img.shape[0]), int(img.shape[1])
    if out is None:
        out = torch.empty_like(img)
    elif out.dtype != torch.uint8 or out.shape != img.shape or not out.is_cuda or not out.is_contiguous():
        raise _hip.HipError("image_augment: out must be a contiguous uint8 device tensor of shape %s" % (tuple(img.shape),))
    flip, stages = image_augment_stages(aug, h, w)
    if len(stages) > IMG_MAX_STAGES:
        raise _hip.HipError("image_augment: %d stages, at most %d" % (len(stages), IMG_MAX_STAGES))
    nbytes = lib.frcnn_image_augment_ws_bytes(h, w)
    if scratch is None and len(stages) > 1:
        scratch = _workspace(nbytes, img.device)
    if scratch is not None and (scratch.dtype != torch.uint8 or not scratch.is_cuda or not scratch.is_contiguous()):
        raise _hip.HipError("image_augment: scratch must be a contiguous uint8 device tensor")
    if debug_pre is not None and (_dev_f32(debug_pre, "debug_pre").numel() != img.numel()):
        raise _hip.HipError("image_augment: debug_pre must hold H*W*3 floats")
    codes = (ctypes.c_int * max(len(stages), 1))(*[c for c, _ in stages])
    flat = []
    for _, vals in stages:
        flat += [float(v) for v in vals] + [0.0] * (IMG_NUM_PARAMS - len(vals))
    _hip.check(lib.frcnn_image_augment(_ptr(img), h, w, int(flip), len(stages), codes, _hip.float_array(flat or [0.0]),
                                       int(aug.seed) & 0xFFFFFFFF, _seed_dev(seed_dev), _ptr(scratch),
                                       0 if scratch is None else scratch.numel(), _ptr(out), _ptr(debug_pre), _stream()),
               "frcnn_image_augment")
    return out


# frcnn_image_spatter: what the kernel's halo holds (include/frcnn_hip.h FRCNN_SPATTER_MAX_TAPS*)
SPATTER_MAX_TAPS = (9, 13)


def image_spatter(img, spatter, out=None, seed_dev=None, debug_liquid=None, debug_mask=None):
    """Test-time Spatter corruption in front of ``prep_im_for_blob`` (frcnn_image_spatter; lib/roi_data_layer/minibatch.py:
    648-664).  ``img``: uint8 (H, W, 3) device tensor in cv2.imread order; ``spatter``: the record
    (``roi_data_layer.image_augment.Spatter`` or any object with ``severity`` and ``seed``; severities 1-3 raise
    NotImplementedError).  Returns the corrupted uint8 frame (``out`` or a new tensor; ``out`` must not be ``img``).
    ``debug_liquid`` / ``debug_mask``: float32 (H, W) device tensors receiving the field after the first blur and the mask
    before its 0.8 cut (tests)."""
    from .roi_data_layer.image_augment import spatter_params, spatter_taps
    params = spatter_params(int(spatter.severity))
    lib = _hip.load()
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise _hip.HipError("image_spatter: img must be a tensor on the MI355X (got %s); this package has no CPU path"
                            % (getattr(img, "device", type(img)),))
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous():
        raise _hip.HipError("image_spatter: img must be a contiguous uint8 (H, W, 3) frame, got %s %s"
                            % (img.dtype, tuple(img.shape)))
    h, w = int(img.shape[0]), int(img.shape[1])
    if out is None:
        out = torch.empty_like(img)
    elif out.dtype != torch.uint8 or out.shape != img.shape or not out.is_cuda or not out.is_contiguous():
        raise _hip.HipError("image_spatter: out must be a contiguous uint8 device tensor of shape %s" % (tuple(img.shape),))
    for name, dbg in (("debug_liquid", debug_liquid), ("debug_mask", debug_mask)):
        if dbg is not None and _dev_f32(dbg, name).numel() != h * w:
            raise _hip.HipError("image_spatter: %s must hold H*W floats" % name)
    taps1, taps2 = spatter_taps(params[2]), spatter_taps(params[4])
    _hip.check(lib.frcnn_image_spatter(_ptr(img), h, w, _hip.float_array(params), _hip.float_array(taps1), len(taps1),
                                       _hip.float_array(taps2), len(taps2), int(spatter.seed) & 0xFFFFFFFF,
                                       _seed_dev(seed_dev), _ptr(out), _ptr(debug_liquid), _ptr(debug_mask), _stream()),
               "frcnn_image_spatter")
    return out


# frcnn_eval_match: eval types, verdict codes and the kernel's two sizes (include/frcnn_hip.h FRCNN_EVAL_*)
EVAL_TYPES = {'2d': 0, 'bev_aa': 1, 'bev': 2, '3d': 3}
EVAL_NONE, EVAL_TP, EVAL_DUP_FP, EVAL_FP = 0, 1, 2, 3
EVAL_CHUNK, EVAL_LDS_GT = 64, 2048


def eval_match(det_boxes, det_rows, det_offsets, gt_boxes, gt_ignore, gt_difficulty, gt_offsets, eval_type, ovthresh,
               ovthresh_dc=0.5, dc_boxes=None, dc_offsets=None, max_gt_per_frame=None):
    """Overlaps and matching of one class's detections against the ground truth, all frames in one launch
    (frcnn_eval_match; lib/datasets/waymo_eval.py:131-213 and the same loop of kitti_eval.py / cadc_eval.py).
    Device tensors grouped by frame: ``det_boxes`` (D, E) float64 with E = 4 for '2d' and 7 otherwise, ``det_rows`` (D,)
    int32, ``gt_boxes`` (G, E) float64, ``gt_ignore`` (G,) uint8 or bool, ``gt_difficulty`` (G,) int32, the offsets
    (F + 1,) int32; ``dc_boxes`` (C, E) / ``dc_offsets`` or None.  ``max_gt_per_frame``: the largest gt count of a frame
    (read back from ``gt_offsets`` when not given: one host synchronisation).
    Returns ``(code, jmax, ovmax, ovmax_dc, det_difficulty, hit)``: int32, int32, float64, float64, int32 per detection
    and uint8 per gt box."""
    lib = _hip.load()
    if eval_type not in EVAL_TYPES:
        raise _hip.HipError("eval_match: eval_type %r, one of %s" % (eval_type, sorted(EVAL_TYPES)))
    elem = 4 if eval_type == '2d' else 7

    def dev(t, name, dtypes, cols=None):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _hip.HipError("eval_match: %s must be a tensor on the MI355X (got %s); this package has no CPU path"
                                % (name, getattr(t, "device", type(t))))
        if t.dtype not in dtypes or not t.is_contiguous():
            raise _hip.HipError("eval_match: %s must be contiguous %s (got %s)" % (name, dtypes[0], t.dtype))
        if (t.dim() != 1) if cols is None else (t.dim() != 2 or t.shape[1] != cols):
            raise _hip.HipError("eval_match: %s must have shape %s for eval_type %r, got %s"
                                % (name, "(n,)" if cols is None else "(n, %d)" % cols, eval_type, tuple(t.shape)))
        return t

    dev(det_boxes, "det_boxes", (torch.float64,), elem)
    dev(gt_boxes, "gt_boxes", (torch.float64,), elem)
    num_det, num_gt = int(det_boxes.shape[0]), int(gt_boxes.shape[0])
    dev(det_rows, "det_rows", (torch.int32,))
    dev(gt_ignore, "gt_ignore", (torch.uint8, torch.bool))
    dev(gt_difficulty, "gt_difficulty", (torch.int32,))
    dev(det_offsets, "det_offsets", (torch.int32,))
    dev(gt_offsets, "gt_offsets", (torch.int32,))
    num_frames = int(det_offsets.numel()) - 1
    if num_frames < 0 or gt_offsets.numel() != num_frames + 1:
        raise _hip.HipError("eval_match: det_offsets and gt_offsets must both hold frames + 1 entries (got %d and %d)"
                            % (det_offsets.numel(), gt_offsets.numel()))
    if det_rows.numel() != num_det or gt_ignore.numel() != num_gt or gt_difficulty.numel() != num_gt:
        raise _hip.HipError("eval_match: det_rows / gt_ignore / gt_difficulty must have one entry per box")
    if (dc_boxes is None) != (dc_offsets is None):
        raise _hip.HipError("eval_match: dc_boxes and dc_offsets go together")
    num_dc = 0
    if dc_boxes is not None:
        dev(dc_boxes, "dc_boxes", (torch.float64,), elem)
        dev(dc_offsets, "dc_offsets", (torch.int32,))
        num_dc = int(dc_boxes.shape[0])
        if dc_offsets.numel() != num_frames + 1:
            raise _hip.HipError("eval_match: dc_offsets must hold frames + 1 entries")
    if max_gt_per_frame is None:
        max_gt_per_frame = int((gt_offsets[1:] - gt_offsets[:-1]).max().item()) if num_frames > 0 else 0
    device = det_boxes.device
    code = torch.empty(num_det, dtype=torch.int32, device=device)
    jmax = torch.empty(num_det, dtype=torch.int32, device=device)
    ovmax = torch.empty(num_det, dtype=torch.float64, device=device)
    ovmax_dc = torch.empty(num_det, dtype=torch.float64, device=device)
    dif = torch.empty(num_det, dtype=torch.int32, device=device)
    hit = torch.zeros(num_gt, dtype=torch.uint8, device=device)
    nbytes = lib.frcnn_eval_match_ws_bytes(num_gt, int(max_gt_per_frame))
    ws = _workspace(nbytes, device) if nbytes else None
    _hip.check(lib.frcnn_eval_match(_ptr(det_boxes), _ptr(det_rows), _ptr(det_offsets), num_det, _ptr(gt_boxes),
                                    _ptr(gt_ignore), _ptr(gt_difficulty), _ptr(gt_offsets), num_gt, _ptr(dc_boxes),
                                    _ptr(dc_offsets), num_dc, num_frames, EVAL_TYPES[eval_type], float(ovthresh),
                                    float(ovthresh_dc), int(max_gt_per_frame), _ptr(code), _ptr(jmax), _ptr(ovmax),
                                    _ptr(ovmax_dc), _ptr(dif), _ptr(hit), _ptr(ws), nbytes, _stream()),
               "frcnn_eval_match")
    return code, jmax, ovmax, ovmax_dc, dif, hit


# frcnn_coco_match: the kernel's three sizes (include/frcnn_hip.h FRCNN_COCO_*)
COCO_PAIRS_PER_WG, COCO_LDS_IOUS, COCO_MASK_GT = 4, 1024, 64


def coco_match(det, det_offsets, gt, gt_crowd, gt_offsets, iou_thrs, area_rng, out=None, ws=None):
    """COCO bbox matching of every (image, category) pair in one launch (frcnn_coco_match; the call lib/datasets/coco.py:251-258
    makes through pycocotools' COCOeval.evaluate, restated in datasets/coco_eval.py).
    Device tensors: ``det`` (D, 5) float64 [x, y, w, h, area], each pair's detections in descending score order and cut to
    the largest maxDets; ``gt`` (G, 5) float64 in annotation order; ``gt_crowd`` (G,) uint8 or bool.
    HOST int32 arrays (numpy or CPU tensors), because the host made them and the checks below read them without a device
    round trip: ``det_offsets`` / ``gt_offsets`` (P + 1,), ascending inside [0, D] / [0, G]; rows that no pair owns are left alone.  ``iou_thrs`` (T,) and ``area_rng``
    (A, 2): float64, host or device, used as they are (np.linspace is never recomputed).
    ``out``: None, or (ious, dt_match, dt_ignore, gt_ignore) device tensors of the shapes below (tests: views between
    guard bands); ``ws``: None or a workspace of frcnn_coco_match_ws_bytes bytes.
    Returns ``(ious, iou_offsets, dt_match, dt_ignore, gt_ignore)``: float64 (sum of D_p * G_p,) with pair p's D_p x G_p
    matrix at the host int64 array ``iou_offsets[p]``, int32 (D, A, T) matched box inside the pair or -1, uint8 (D, A, T),
    uint8 (G, A).  No host synchronisation."""
    lib = _hip.load()

    def dev(t, name, dtypes, cols=None):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _hip.HipError("coco_match: %s must be a tensor on the MI355X (got %s); this package has no CPU path"
                                % (name, getattr(t, "device", type(t))))
        if t.dtype not in dtypes or not t.is_contiguous():
            raise _hip.HipError("coco_match: %s must be contiguous %s (got %s)" % (name, dtypes[0], t.dtype))
        if (t.dim() != 1) if cols is None else (t.dim() != 2 or t.shape[1] != cols):
            raise _hip.HipError("coco_match: %s must have shape %s, got %s"
                                % (name, "(n,)" if cols is None else "(n, %d)" % cols, tuple(t.shape)))
        return t

    def host_offsets(o, name, total):
        if isinstance(o, torch.Tensor):
            if o.is_cuda:
                raise _hip.HipError("coco_match: %s must be a HOST integer array (it is checked before the launch)" % name)
            o = o.numpy()
        o = np.asarray(o)
        if o.dtype.kind not in "iu" or o.ndim != 1 or o.size < 1:
            raise _hip.HipError("coco_match: %s must be a host integer array of pairs + 1 entries" % name)
        o = o.astype(np.int64)
        if o[0] < 0 or o[-1] > total or (np.diff(o) < 0).any():
            raise _hip.HipError("coco_match: %s must ascend inside [0, %d]" % (name, total))
        return o

    dev(det, "det", (torch.float64,), 5)
    dev(gt, "gt", (torch.float64,), 5)
    device = det.device
    num_det, num_gt = int(det.shape[0]), int(gt.shape[0])
    dev(gt_crowd, "gt_crowd", (torch.uint8, torch.bool))
    if gt_crowd.numel() != num_gt:
        raise _hip.HipError("coco_match: gt_crowd must have one entry per box")
    d_off = host_offsets(det_offsets, "det_offsets", num_det)
    g_off = host_offsets(gt_offsets, "gt_offsets", num_gt)
    if d_off.size != g_off.size:
        raise _hip.HipError("coco_match: det_offsets and gt_offsets must both hold pairs + 1 entries (got %d and %d)"
                            % (d_off.size, g_off.size))
    num_pairs = d_off.size - 1
    n_d, n_g = np.diff(d_off), np.diff(g_off)
    i_off = np.zeros(num_pairs + 1, dtype=np.int64)
    np.cumsum(n_d * n_g, out=i_off[1:])
    num_iou = int(i_off[-1])
    max_gt = int(n_g.max()) if num_pairs else 0

    def small(a, name, shape_ok):
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
        if a.dtype != torch.float64 or not shape_ok(a) or a.numel() == 0:
            raise _hip.HipError("coco_match: %s must be float64 of shape %s" % (name, "(T,)" if name == "iou_thrs" else "(A, 2)"))
        return a.contiguous().to(device, non_blocking=True)

    thr = small(iou_thrs, "iou_thrs", lambda a: a.dim() == 1)
    rng = small(area_rng, "area_rng", lambda a: a.dim() == 2 and a.shape[1] == 2)
    num_thr, num_area = int(thr.numel()), int(rng.shape[0])
    shapes = ((num_iou,), (num_det, num_area, num_thr), (num_det, num_area, num_thr), (num_gt, num_area))
    dtypes = (torch.float64, torch.int32, torch.uint8, torch.uint8)
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=device) for s, d in zip(shapes, dtypes))
    else:
        if len(out) != 4:
            raise _hip.HipError("coco_match: out is (ious, dt_match, dt_ignore, gt_ignore)")
        for t, s, d, name in zip(out, shapes, dtypes, ("ious", "dt_match", "dt_ignore", "gt_ignore")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != d or tuple(t.shape) != s or not t.is_contiguous():
                raise _hip.HipError("coco_match: out %s must be a contiguous %s device tensor of shape %s" % (name, d, s))
    ious, dt_match, dt_ignore, gt_ignore = out
    up = [torch.from_numpy(o).to(device, non_blocking=True) for o in (d_off.astype(np.int32), g_off.astype(np.int32), i_off)]
    nbytes = lib.frcnn_coco_match_ws_bytes(num_gt, max_gt, num_area, num_thr)
    ws = _given_workspace("coco_match", ws, nbytes, device)
    _hip.check(lib.frcnn_coco_match(_ptr(det), _ptr(up[0]), num_det, _ptr(gt), _ptr(gt_crowd), _ptr(up[1]), num_gt,
                                    _ptr(up[2]), num_iou, num_pairs, _ptr(thr), num_thr, _ptr(rng), num_area, max_gt,
                                    _ptr(ious), _ptr(dt_match), _ptr(dt_ignore), _ptr(gt_ignore), _ptr(ws), nbytes,
                                    _stream()), "frcnn_coco_match")
    return ious, i_off, dt_match, dt_ignore, gt_ignore


# ----------------------------------------------------------------------------------------------
# training path
# ----------------------------------------------------------------------------------------------
def act_bwd(dy, y=None, scale=None, relu=False, want_res=False):
    """Backward of act(conv*scale + shift + res): returns (d_conv, d_res or None)."""
    lib = _hip.load()
    _dev_f32(dy, "dy")
    k = dy.shape[-1]
    rows = dy.numel() // k
    if relu:
        _dev_f32(y, "y")
    d_conv = torch.empty_like(dy)
    d_res = torch.empty_like(dy) if want_res else None
    _hip.check(lib.frcnn_act_bwd(_ptr(dy), _ptr(y) if relu else None, _ptr(scale), int(bool(relu)), rows, k, _ptr(d_conv),
                                 _ptr(d_res), _stream()), "frcnn_act_bwd")
    return d_conv, d_res


# True: the statistics / coefficient pass of frcnn_bn_train_fwd / _bwd runs inside the column-sum kernel (tile counters as for
# the filter gradients); False: as a launch of its own (A/B, and the arithmetic is the same code: bit-identical)
BN_FUSED_FINAL = os.environ.get('FRCNN_BN_FUSED_FINAL', '1') != '0'


def bn_train_fwd(y, gamma, beta, eps, momentum, running_mean=None, running_var=None, residual=None, relu=False):
    """BatchNorm with batch statistics over the rows of an NHWC tensor (+ residual, ReLU); the running statistics are
    updated in place.  Returns (out, save_mean, save_invstd)."""
    lib = _hip.load()
    _dev_f32(y, "y")
    c = y.shape[-1]
    rows = y.numel() // c
    for nm, t in (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var)):
        if t is not None:
            _dev_f32(t, nm)
            if t.numel() != c:
                raise _hip.HipError("bn_train_fwd: %s has %d elements, expected %d" % (nm, t.numel(), c))
    if residual is not None:
        _dev_f32(residual, "residual")
        if residual.shape != y.shape:
            raise _hip.HipError("bn_train_fwd: residual %s vs %s" % (tuple(residual.shape), tuple(y.shape)))
    out = torch.empty_like(y)
    mean = torch.empty((c,), dtype=torch.float32, device=y.device)
    invstd = torch.empty_like(mean)
    nbytes = lib.frcnn_bn_train_ws_bytes(c)
    ws = _workspace(nbytes, y.device)
    counters = _tile_counters(y.device, lib.frcnn_bn_train_counters(c)) if BN_FUSED_FINAL else None
    _hip.check(lib.frcnn_bn_train_fwd(_ptr(y), rows, c, _ptr(gamma), _ptr(beta), float(eps), float(momentum),
                                      _ptr(running_mean), _ptr(running_var), _ptr(residual), int(bool(relu)), _ptr(out),
                                      _ptr(mean), _ptr(invstd), _ptr(ws), nbytes, _ptr(counters), _stream()),
               "frcnn_bn_train_fwd")
    return out, mean, invstd


def bn_train_bwd(dout, out, y, gamma, save_mean, save_invstd, relu=False, want_res=False, grad_gamma=None, grad_beta=None):
    """Backward of bn_train_fwd: returns (dy, dres or None, dgamma, dbeta).  ``grad_gamma`` / ``grad_beta`` (both or neither):
    the parameters' own (c,) gradient buffers - the sums are ADDED into them and returned as dgamma / dbeta."""
    lib = _hip.load()
    _dev_f32(dout, "dout"); _dev_f32(y, "y"); _dev_f32(save_mean, "save_mean"); _dev_f32(save_invstd, "save_invstd")
    if relu:
        _dev_f32(out, "out")
    c = y.shape[-1]
    rows = y.numel() // c
    if dout.shape != y.shape or save_mean.numel() != c or save_invstd.numel() != c:
        raise _hip.HipError("bn_train_bwd: shape mismatch")
    dy = torch.empty_like(y)
    dres = torch.empty_like(y) if want_res else None
    accumulate = grad_gamma is not None
    if accumulate:
        if grad_beta is None or grad_gamma.numel() != c or grad_beta.numel() != c:
            raise _hip.HipError("bn_train_bwd: grad_gamma and grad_beta must both be (c,) gradient buffers")
        dgamma, dbeta = _dev_f32(grad_gamma, "grad_gamma"), _dev_f32(grad_beta, "grad_beta")
    else:
        dgamma = torch.empty((c,), dtype=torch.float32, device=y.device)
        dbeta = torch.empty_like(dgamma)
    nbytes = lib.frcnn_bn_train_ws_bytes(c)
    ws = _workspace(nbytes, y.device)
    counters = _tile_counters(y.device, lib.frcnn_bn_train_counters(c)) if BN_FUSED_FINAL else None
    _hip.check(lib.frcnn_bn_train_bwd(_ptr(dout), _ptr(out) if relu else None, _ptr(y), rows, c, _ptr(gamma),
                                      _ptr(save_mean), _ptr(save_invstd), int(bool(relu)), _ptr(dy), _ptr(dres),
                                      _ptr(dgamma), _ptr(dbeta), int(accumulate), _ptr(ws), nbytes, _ptr(counters), _stream()),
               "frcnn_bn_train_bwd")
    return dy, dres, dgamma, dbeta


def upsample_bilinear_add(x, lateral):
    """F.interpolate(x, size=lateral.shape[1:3], mode='bilinear', align_corners=False) + lateral, NHWC."""
    lib = _hip.load()
    _dev_f32(x, "x"); _dev_f32(lateral, "lateral")
    n, h, w, c = x.shape
    n2, oh, ow, c2 = lateral.shape
    if n2 != n or c2 != c:
        raise _hip.HipError("upsample_bilinear_add: %s vs %s" % (tuple(x.shape), tuple(lateral.shape)))
    out = torch.empty_like(lateral)
    _hip.check(lib.frcnn_upsample_bilinear_add_fwd(_ptr(x), _ptr(lateral), _ptr(out), n, h, w, oh, ow, c, _stream()),
               "frcnn_upsample_bilinear_add_fwd")
    return out


def upsample_bilinear_bwd(dout, in_hw):
    lib = _hip.load()
    _dev_f32(dout, "dout")
    n, oh, ow, c = dout.shape
    h, w = in_hw
    dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dout.device)
    _hip.check(lib.frcnn_upsample_bilinear_bwd(_ptr(dout), _ptr(dx), n, h, w, oh, ow, c, _stream()),
               "frcnn_upsample_bilinear_bwd")
    return dx


ROI_ALIGN_BWD_PLANNED = True      # False: always the sample-by-sample backward (frcnn_roi_align_bwd)


def roi_align_bwd(dout, feat_shape, rois, spatial_scale, sampling_ratio=0, roi_count=None, level_of_roi=None, level=-1,
                  dfeat=None):
    """Scatter dout (R,P,P,C) into dfeat (1,H,W,C) (created zero-filled unless given, then accumulated into).  7x7 bins and
    C % 4 == 0 go through the forward's plan (frcnn_roi_align_bwd_planned), anything else sample by sample."""
    lib = _hip.load()
    _dev_f32(dout, "dout"); _dev_f32(rois, "rois")
    _, h, w, c = feat_shape
    r, p = dout.shape[0], dout.shape[1]
    if dfeat is None:
        dfeat = torch.zeros(tuple(feat_shape), dtype=torch.float32, device=dout.device)
    if ROI_ALIGN_BWD_PLANNED and feat_shape[0] == 1 and c % 4 == 0:
        ws_bytes = lib.frcnn_roi_align_fwd_ws_bytes(h, w, c, r, p)
        if ws_bytes:
            ws = _workspace(ws_bytes, dout.device)
            _hip.check(lib.frcnn_roi_align_bwd_planned(_ptr(dout), h, w, c, _ptr(rois), _ptr(roi_count), r, p,
                                                       float(spatial_scale), int(sampling_ratio), _ptr(level_of_roi), int(level),
                                                       _ptr(dfeat), _ptr(ws), ws_bytes, _stream()),
                       "frcnn_roi_align_bwd_planned")
            return dfeat
    _hip.check(lib.frcnn_roi_align_bwd(_ptr(dout), h, w, c, _ptr(rois), _ptr(roi_count), r, p, float(spatial_scale),
                                       int(sampling_ratio), _ptr(level_of_roi), int(level), _ptr(dfeat), _stream()),
               "frcnn_roi_align_bwd")
    return dfeat


def labelled_pixels(labels, hw, num_anchors, cap):
    """labels (hw * A,) in (H,W,A) order -> (idx int64 (cap,), count int32 (2,) = [min(total, cap), total]): the pixels that
    carry at least one anchor with a label != -1, ascending; -1 beyond the count (frcnn_labelled_pixels)."""
    lib = _hip.load()
    _dev_f32(labels, "labels")
    if labels.numel() != hw * num_anchors:
        raise _hip.HipError("labelled_pixels: labels has %d elements, expected %d x %d" % (labels.numel(), hw, num_anchors))
    idx = torch.empty((cap,), dtype=torch.int64, device=labels.device)
    count = torch.empty((2,), dtype=torch.int32, device=labels.device)
    ws_bytes = lib.frcnn_labelled_pixels_ws_bytes(hw)
    ws = _workspace(ws_bytes, labels.device)
    _hip.check(lib.frcnn_labelled_pixels(_ptr(labels), hw, num_anchors, cap, _ptr(idx), _ptr(count), _ptr(ws), ws_bytes,
                                         _stream()), "frcnn_labelled_pixels")
    return idx, count


def gather_patches(x, idx, count, r, s, pad):
    """x (1,H,W,C), idx (cap,) pixels -> (cap, r, s, C): the r x s windows around the listed pixels (frcnn_gather_patches)."""
    lib = _hip.load()
    _dev_f32(x, "x")
    n, h, w, c = x.shape
    if n != 1:
        raise _hip.HipError("gather_patches: one image per call")
    cap = idx.numel()
    out = torch.empty((cap, r, s, c), dtype=torch.float32, device=x.device)
    _hip.check(lib.frcnn_gather_patches(_ptr(x), h, w, c, _ptr(idx), _ptr(count), cap, r, s, pad, _ptr(out), _stream()),
               "frcnn_gather_patches")
    return out


def scatter_add_patches(d, idx, count, h, w, pad, out=None):
    """Adjoint of gather_patches: d (cap, r, s, C) -> dx (1,h,w,C) (zero-filled here unless ``out`` is given; float atomics)."""
    lib = _hip.load()
    _dev_f32(d, "d")
    cap, r, s, c = d.shape
    if out is None:
        out = torch.zeros((1, h, w, c), dtype=torch.float32, device=d.device)
    _hip.check(lib.frcnn_scatter_add_patches(_ptr(d), h, w, c, _ptr(idx), _ptr(count), cap, r, s, pad, _ptr(out), _stream()),
               "frcnn_scatter_add_patches")
    return out


def rpn_loss(rpn, num_anchors, labels, targets, inside, outside, grad_ce=1.0, grad_box=1.0, want_grad=True):
    """rpn (HW, ld) fused head output.  Returns (losses (3,) [ce, box, count], drpn or None)."""
    lib = _hip.load()
    for nm, t in (("rpn", rpn), ("labels", labels), ("targets", targets), ("inside", inside), ("outside", outside)):
        _dev_f32(t, nm)
    hw, ld = rpn.shape
    losses = torch.empty((3,), dtype=torch.float32, device=rpn.device)
    drpn = torch.empty_like(rpn) if want_grad else None
    ws_bytes = lib.frcnn_rpn_loss_ws_bytes()
    ws = _workspace(ws_bytes, rpn.device)
    _hip.check(lib.frcnn_rpn_loss(_ptr(rpn), ld, num_anchors, hw, _ptr(labels), _ptr(targets), _ptr(inside), _ptr(outside),
                                  float(grad_ce), float(grad_box), _ptr(losses), _ptr(drpn), _ptr(ws), ws_bytes, _stream()),
               "frcnn_rpn_loss")
    return losses, drpn


def det_loss(cls_score, labels, bbox_pred, targets, inside, outside, bbox_elem=4, grad_ce=1.0, grad_box=1.0,
             want_grad=True, lidar=None):
    """Returns (losses (2,) [ce, box], dcls, dbox).  ``lidar=(reg_loss_weight[7], ry_sin)`` selects the 7-element LiDAR
    form (sin() on the yaw difference, per-element weights)."""
    lib = _hip.load()
    for nm, t in (("cls_score", cls_score), ("labels", labels), ("bbox_pred", bbox_pred), ("targets", targets),
                  ("inside", inside), ("outside", outside)):
        _dev_f32(t, nm)
    r, k = cls_score.shape
    losses = torch.empty((2,), dtype=torch.float32, device=cls_score.device)
    dcls = torch.empty_like(cls_score) if want_grad else None
    dbox = torch.empty_like(bbox_pred) if want_grad else None
    if lidar is not None:
        weights, ry_sin = lidar
        if bbox_pred.shape[1] != 7 * k:
            raise _hip.HipError("det_loss: LiDAR bbox_pred must be (R, 7*K), got %s" % (tuple(bbox_pred.shape),))
        _hip.check(lib.frcnn_det_loss_lidar(_ptr(cls_score), _ptr(labels), r, k, _ptr(bbox_pred), _ptr(targets),
                                            _ptr(inside), _ptr(outside), _hip.float_array([float(v) for v in weights]),
                                            int(bool(ry_sin)), float(grad_ce), float(grad_box), _ptr(losses), _ptr(dcls),
                                            _ptr(dbox), _stream()), "frcnn_det_loss_lidar")
        return losses, dcls, dbox
    _hip.check(lib.frcnn_det_loss(_ptr(cls_score), _ptr(labels), r, k, _ptr(bbox_pred), _ptr(targets), _ptr(inside),
                                  _ptr(outside), int(bbox_elem), float(grad_ce), float(grad_box), _ptr(losses), _ptr(dcls),
                                  _ptr(dbox), _stream()), "frcnn_det_loss")
    return losses, dcls, dbox


def det_loss_aleatoric(cls_score, labels, bbox_pred, bbox_var, targets, inside, outside, bbox_elem=4, weights=None,
                       ry_sin=False, grad_ce=1.0, grad_box=1.0):
    """Detection losses with the aleatoric attenuation (loss_utils.py:82-85).  Returns (losses (2,), dcls, dbox, dvar)."""
    lib = _hip.load()
    for nm, t in (("cls_score", cls_score), ("labels", labels), ("bbox_pred", bbox_pred), ("bbox_var", bbox_var),
                  ("targets", targets), ("inside", inside), ("outside", outside)):
        _dev_f32(t, nm)
    r, k = cls_score.shape
    if bbox_pred.shape != (r, bbox_elem * k) or bbox_var.shape != bbox_pred.shape:
        raise _hip.HipError("det_loss_aleatoric: bbox_pred / bbox_var must be (R, %d*K)" % bbox_elem)
    losses = torch.empty((2,), dtype=torch.float32, device=cls_score.device)
    dcls, dbox, dvar = torch.empty_like(cls_score), torch.empty_like(bbox_pred), torch.empty_like(bbox_var)
    w = _hip.float_array([float(v) for v in weights]) if weights is not None else None
    _hip.check(lib.frcnn_det_loss_aleatoric(_ptr(cls_score), _ptr(labels), r, k, _ptr(bbox_pred), _ptr(bbox_var),
                                            _ptr(targets), _ptr(inside), _ptr(outside), int(bbox_elem), w,
                                            int(bool(ry_sin)), float(grad_ce), float(grad_box), _ptr(losses), _ptr(dcls),
                                            _ptr(dbox), _ptr(dvar), _stream()), "frcnn_det_loss_aleatoric")
    return losses, dcls, dbox, dvar


def mc_bbox_var(samples):
    """(T, ...) stack of stochastic passes -> unbiased variance over T, clamped at 0 (compute_bbox_var)."""
    lib = _hip.load()
    _dev_f32(samples, "samples")
    t = samples.shape[0]
    out = torch.empty(samples.shape[1:], dtype=torch.float32, device=samples.device)
    _hip.check(lib.frcnn_mc_bbox_var(_ptr(samples), t, out.numel(), _ptr(out), _stream()), "frcnn_mc_bbox_var")
    return out


def mc_cls_stats(cls_score_samples, want_var=False):
    """(T, N, K) logits -> (mean softmax (N,K), entropy (N,), mutual information (N,)[, variance of the softmax over T
    (N,K)]), log base 2."""
    lib = _hip.load()
    _dev_f32(cls_score_samples, "cls_score_samples")
    t, n, k = cls_score_samples.shape
    dev = cls_score_samples.device
    mean_prob = torch.empty((n, k), dtype=torch.float32, device=dev)
    entropy, mi = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)
    var = torch.empty((n, k), dtype=torch.float32, device=dev) if want_var else None
    _hip.check(lib.frcnn_mc_cls_stats(_ptr(cls_score_samples), t, n, k, _ptr(mean_prob), _ptr(entropy), _ptr(mi),
                                      _ptr(var), _stream()), "frcnn_mc_cls_stats")
    return (mean_prob, entropy, mi, var) if want_var else (mean_prob, entropy, mi)


def mc_mean(samples):
    """(T, ...) -> mean over T (summed in sample order)."""
    lib = _hip.load()
    _dev_f32(samples, "samples")
    out = torch.empty(samples.shape[1:], dtype=torch.float32, device=samples.device)
    _hip.check(lib.frcnn_mc_mean(_ptr(samples), samples.shape[0], out.numel(), _ptr(out), _stream()), "frcnn_mc_mean")
    return out


def _seed_dev(seed_dev):
    """Device word added to the scalar seed (a replayed hipGraph keeps its scalars): int32 / uint32 tensor of one element."""
    if seed_dev is None:
        return None
    if not seed_dev.is_cuda or seed_dev.numel() != 1 or seed_dev.element_size() != 4:
        raise _hip.HipError("seed_dev must be one 32-bit word on the device")
    return seed_dev.data_ptr()


def dropout(x, p, seed, stream_id, repeat=1, seed_dev=None):
    """nn.Dropout(p) in train() mode with counter-based masks; ``repeat`` stochastic copies: x (...) -> (repeat, ...)
    (the leading dimension is dropped for repeat == 1).  The draws use ``seed + *seed_dev``."""
    lib = _hip.load()
    _dev_f32(x, "x")
    shape = tuple(x.shape) if repeat == 1 else (repeat,) + tuple(x.shape)
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    _hip.check(lib.frcnn_dropout_fwd(_ptr(x), x.numel(), int(repeat), float(p), int(seed) & 0xFFFFFFFF, _seed_dev(seed_dev),
                                     int(stream_id) & 0xFFFFFFFF, _ptr(y), _stream()), "frcnn_dropout_fwd")
    return y


def dropout_bwd(dy, p, seed, stream_id, repeat=1, seed_dev=None):
    lib = _hip.load()
    _dev_f32(dy, "dy")
    shape = tuple(dy.shape) if repeat == 1 else tuple(dy.shape[1:])
    dx = torch.empty(shape, dtype=torch.float32, device=dy.device)
    _hip.check(lib.frcnn_dropout_bwd(_ptr(dy), dx.numel(), int(repeat), float(p), int(seed) & 0xFFFFFFFF, _seed_dev(seed_dev),
                                     int(stream_id) & 0xFFFFFFFF, _ptr(dx), _stream()), "frcnn_dropout_bwd")
    return dx


def logit_distort(score, var, num_samples, seed, stream_id, var_is_log=False, seed_dev=None):
    """logit_distort (loss_utils.py:143-147): (N,K) logits and (log-)variances -> ((S, N, K) distorted logits, (N,K)
    variances)."""
    lib = _hip.load()
    _dev_f32(score, "score"); _dev_f32(var, "var")
    if score.shape != var.shape:
        raise _hip.HipError("logit_distort: score %s vs var %s" % (tuple(score.shape), tuple(var.shape)))
    out = torch.empty((int(num_samples),) + tuple(score.shape), dtype=torch.float32, device=score.device)
    var_out = torch.empty_like(var)
    _hip.check(lib.frcnn_logit_distort(_ptr(score), _ptr(var), score.numel(), int(num_samples), int(seed) & 0xFFFFFFFF,
                                       _seed_dev(seed_dev), int(stream_id) & 0xFFFFFFFF, int(bool(var_is_log)), _ptr(out), _ptr(var_out),
                                       _stream()), "frcnn_logit_distort")
    return out, var_out


def exp(x):
    lib = _hip.load()
    _dev_f32(x, "x")
    y = torch.empty_like(x)
    _hip.check(lib.frcnn_exp(_ptr(x), x.numel(), _ptr(y), _stream()), "frcnn_exp")
    return y


def bayesian_cross_entropy(cls_score, cls_var, labels, num_samples, seed, stream_id, grad=1.0, want_grad=True,
                           var_is_log=False, seed_dev=None):
    """bayesian_cross_entropy (loss_utils.py:149-169).  Returns (loss (1,), dscore, dvar) (gradients scaled by grad).
    One thread per RoI, at most 16 classes; ``bayesian_cross_entropy_wide`` takes any class count."""
    return _bayesian_cross_entropy("frcnn_bayesian_cross_entropy", cls_score, cls_var, labels, num_samples, seed, stream_id,
                                   grad, want_grad, var_is_log, seed_dev)[:3]


def _bayesian_cross_entropy(entry, cls_score, cls_var, labels, num_samples, seed, stream_id, grad, want_grad, var_is_log,
                            seed_dev):
    lib = _hip.load()
    _dev_f32(cls_score, "cls_score"); _dev_f32(cls_var, "cls_var"); _dev_f32(labels, "labels")
    n, k = cls_score.shape
    if tuple(cls_var.shape) != (n, k) or labels.numel() != n:
        raise _hip.HipError("%s: score %s, var %s, %d labels" % (entry[6:], tuple(cls_score.shape), tuple(cls_var.shape),
                                                                 labels.numel()))
    dev = cls_score.device
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    per_roi = torch.empty((n,), dtype=torch.float32, device=dev)
    dscore = torch.empty_like(cls_score) if want_grad else None
    dvar = torch.empty_like(cls_var) if want_grad else None
    _hip.check(getattr(lib, entry)(_ptr(cls_score), _ptr(cls_var), _ptr(labels), n, k, int(num_samples),
                                   int(seed) & 0xFFFFFFFF, _seed_dev(seed_dev), int(stream_id) & 0xFFFFFFFF,
                                   int(bool(var_is_log)), float(grad), _ptr(loss), _ptr(per_roi), _ptr(dscore), _ptr(dvar),
                                   _stream()), entry)
    return loss, dscore, dvar, per_roi


BAYES_CE_NARROW_MAX_CLASSES = 16       # KMAX of bayes_ce_kernel (csrc/train_ops.hip)
BAYES_CE_WIDE_MAX_CLASSES = 1024       # BAYES_WIDE_MAX_CLASSES


def bayes_ce_uses_wide_form(num_classes):
    """The rule nets/uncertainty._DetLossUcFn follows: the one-thread-per-RoI kernel wherever it accepts the class count
    (every detector that trained before launches the kernel it launched before), the one-wave-per-RoI kernel above."""
    return int(num_classes) > BAYES_CE_NARROW_MAX_CLASSES


def bayesian_cross_entropy_wide(cls_score, cls_var, labels, num_samples, seed, stream_id, grad=1.0, want_grad=True,
                                var_is_log=False, seed_dev=None, want_per_roi=False):
    """``bayesian_cross_entropy`` for 2 <= classes <= 1024: one wavefront per RoI, the same draws and the same order of
    every sum, so both give the same bits where both accept the class count.  ``want_per_roi`` appends the (N,) per-RoI
    losses the mean is taken over."""
    out = _bayesian_cross_entropy("frcnn_bayesian_cross_entropy_wide", cls_score, cls_var, labels, num_samples, seed,
                                  stream_id, grad, want_grad, var_is_log, seed_dev)
    return out if want_per_roi else out[:3]


def bbox_overlaps(boxes, query_boxes):
    """IoU (+1 convention) between boxes (N, >=4) and query_boxes (K, >=4) -> (N, K)."""
    lib = _hip.load()
    _dev_f32(boxes, "boxes"); _dev_f32(query_boxes, "query_boxes")
    n, k = boxes.shape[0], query_boxes.shape[0]
    out = torch.empty((n, k), dtype=torch.float32, device=boxes.device)
    if n and k:
        _hip.check(lib.frcnn_bbox_overlaps(_ptr(boxes), boxes.shape[1], n, _ptr(query_boxes), query_boxes.shape[1], k,
                                           _ptr(out), _stream()), "frcnn_bbox_overlaps")
    return out


def bbox_transform(ex_rois, gt_rois):
    """Row-wise regression targets (N,4) of gt_rois (N, >=4) against ex_rois (N, >=4) (bbox_transform.py:52-70)."""
    lib = _hip.load()
    _dev_f32(ex_rois, "ex_rois"); _dev_f32(gt_rois, "gt_rois")
    n = ex_rois.shape[0]
    if gt_rois.shape[0] != n:
        raise _hip.HipError("bbox_transform: %d ex_rois vs %d gt_rois" % (n, gt_rois.shape[0]))
    out = torch.empty((n, 4), dtype=torch.float32, device=ex_rois.device)
    if n:
        _hip.check(lib.frcnn_bbox_transform(_ptr(ex_rois), ex_rois.shape[1], _ptr(gt_rois), gt_rois.shape[1], n, _ptr(out),
                                            _stream()), "frcnn_bbox_transform")
    return out


def lidar_bbox_transform(ex_rois, ex_anchors_3d, gt_rois):
    """Row-wise 7-DoF regression targets (N,7) (bbox_transform.py:16-49)."""
    lib = _hip.load()
    _dev_f32(ex_rois, "ex_rois"); _dev_f32(ex_anchors_3d, "ex_anchors_3d"); _dev_f32(gt_rois, "gt_rois")
    n = ex_rois.shape[0]
    if gt_rois.shape[0] != n or ex_anchors_3d.shape[0] != n or ex_anchors_3d.shape[1] != 7:
        raise _hip.HipError("lidar_bbox_transform: row counts / anchor width do not match")
    out = torch.empty((n, 7), dtype=torch.float32, device=ex_rois.device)
    if n:
        _hip.check(lib.frcnn_lidar_bbox_transform(_ptr(ex_rois), ex_rois.shape[1], _ptr(ex_anchors_3d), _ptr(gt_rois),
                                                  gt_rois.shape[1], n, _ptr(out), _stream()), "frcnn_lidar_bbox_transform")
    return out


def _gt_count(gt_count):
    if gt_count is None:
        return None
    if not gt_count.is_cuda or gt_count.dtype != torch.int32 or gt_count.numel() != 1:
        raise _hip.HipError("gt_count must be a one-element int32 device tensor")
    return gt_count.data_ptr()


def anchor_target_layer(anchors, gt_boxes, info, rpn_batchsize, fg_fraction, neg_ov, pos_ov, seed, seed_dev=None,
                        gt_count=None):
    """Returns labels (N,), targets/inside/outside (N,4) in anchor order and counts (2,) int32 [fg, bg candidates].
    ``gt_count`` (int32 device tensor): live rows of a ``gt_boxes`` buffer padded to its row count."""
    lib = _hip.load()
    _dev_f32(anchors, "anchors"); _dev_f32(gt_boxes, "gt_boxes")
    n, g = anchors.shape[0], gt_boxes.shape[0]
    if gt_boxes.shape[1] != 5:
        raise _hip.HipError("anchor_target_layer: gt_boxes must be (G,5)")
    dev = anchors.device
    labels = torch.empty((n,), dtype=torch.float32, device=dev)
    targets, inside, outside = (torch.empty((n, 4), dtype=torch.float32, device=dev) for _ in range(3))
    counts = torch.zeros((2,), dtype=torch.int32, device=dev)
    ws_bytes = lib.frcnn_anchor_target_layer_ws_bytes(n, g, int(rpn_batchsize))
    ws = _workspace(ws_bytes, dev)
    _hip.check(lib.frcnn_anchor_target_layer(
        _ptr(anchors), n, _ptr(gt_boxes), g, _gt_count(gt_count), _hip.float_array([float(v) for v in list(info)[:4]]),
        int(rpn_batchsize),
        float(fg_fraction), float(neg_ov), float(pos_ov), int(seed) & 0xFFFFFFFF, _ptr(seed_dev), _ptr(labels), _ptr(targets),
        _ptr(inside), _ptr(outside), _ptr(counts), _ptr(ws), ws_bytes, _stream()), "frcnn_anchor_target_layer")
    return labels, targets, inside, outside, counts


def proposal_target_layer(rois, roi_scores, gt_boxes, num_classes, rois_per_frame, fg_fraction, fg_thresh, bg_hi, bg_lo,
                          means, stds, seed, roi_count=None, anchors_3d=None, true_gt_boxes=None, skip_mask=None, seed_dev=None,
                          gt_count=None):
    """Returns dict(labels (R,), rois (R,5), scores (R,), targets/inside/outside (R,4K), assign int32 (R,), counts int32 (4,)).
    With ``anchors_3d`` (num_rois,7) and ``true_gt_boxes`` (G,8) the LiDAR form: 7K-wide targets and ``anchors_3d`` (R,7)."""
    lib = _hip.load()
    _dev_f32(rois, "rois"); _dev_f32(gt_boxes, "gt_boxes")
    if roi_scores is not None:
        _dev_f32(roi_scores, "roi_scores")
    dev = rois.device
    r = int(rois_per_frame)
    if skip_mask is not None and (not skip_mask.is_cuda or skip_mask.dtype != torch.uint8 or
                                  skip_mask.numel() != rois.shape[0] or not skip_mask.is_contiguous()):
        raise _hip.HipError("proposal_target_layer: skip_mask must be a contiguous uint8 device tensor of num_rois bytes")
    if anchors_3d is not None:
        _dev_f32(anchors_3d, "anchors_3d"); _dev_f32(true_gt_boxes, "true_gt_boxes")
        if anchors_3d.shape != (rois.shape[0], 7) or true_gt_boxes.shape != (gt_boxes.shape[0], 8) or gt_boxes.shape[1] != 5:
            raise _hip.HipError("proposal_target_layer: LiDAR form needs anchors_3d (num_rois,7), gt_boxes (G,5), "
                                "true_gt_boxes (G,8)")
        e = 7
        out = {"labels": torch.empty((r,), dtype=torch.float32, device=dev),
               "rois": torch.empty((r, 5), dtype=torch.float32, device=dev),
               "scores": torch.empty((r,), dtype=torch.float32, device=dev),
               "anchors_3d": torch.empty((r, 7), dtype=torch.float32, device=dev),
               "targets": torch.empty((r, e * num_classes), dtype=torch.float32, device=dev),
               "inside": torch.empty((r, e * num_classes), dtype=torch.float32, device=dev),
               "outside": torch.empty((r, e * num_classes), dtype=torch.float32, device=dev),
               "assign": torch.empty((r,), dtype=torch.int32, device=dev),
               "counts": torch.zeros((4,), dtype=torch.int32, device=dev)}
        _hip.check(lib.frcnn_proposal_target_layer_lidar(
            _ptr(rois), _ptr(roi_scores), _ptr(roi_count), rois.shape[0], _ptr(anchors_3d), _ptr(gt_boxes),
            _ptr(true_gt_boxes), gt_boxes.shape[0], _gt_count(gt_count), int(num_classes), r, float(fg_fraction), float(fg_thresh), float(bg_hi),
            float(bg_lo), _hip.float_array(means), _hip.float_array(stds), int(seed) & 0xFFFFFFFF, _ptr(seed_dev), _ptr(out["labels"]),
            _ptr(out["rois"]), _ptr(out["scores"]), _ptr(out["anchors_3d"]), _ptr(out["targets"]), _ptr(out["inside"]),
            _ptr(out["outside"]), _ptr(out["assign"]), _ptr(out["counts"]), _ptr(skip_mask), _stream()),
            "frcnn_proposal_target_layer_lidar")
        return out
    out = {"labels": torch.empty((r,), dtype=torch.float32, device=dev),
           "rois": torch.empty((r, 5), dtype=torch.float32, device=dev),
           "scores": torch.empty((r,), dtype=torch.float32, device=dev),
           "targets": torch.empty((r, 4 * num_classes), dtype=torch.float32, device=dev),
           "inside": torch.empty((r, 4 * num_classes), dtype=torch.float32, device=dev),
           "outside": torch.empty((r, 4 * num_classes), dtype=torch.float32, device=dev),
           "assign": torch.empty((r,), dtype=torch.int32, device=dev),
           "counts": torch.zeros((4,), dtype=torch.int32, device=dev)}
    _hip.check(lib.frcnn_proposal_target_layer(
        _ptr(rois), _ptr(roi_scores), _ptr(roi_count), rois.shape[0], _ptr(gt_boxes), gt_boxes.shape[0], _gt_count(gt_count),
        int(num_classes), r, float(fg_fraction), float(fg_thresh), float(bg_hi), float(bg_lo), _hip.float_array(means),
        _hip.float_array(stds), int(seed) & 0xFFFFFFFF, _ptr(seed_dev), _ptr(out["labels"]), _ptr(out["rois"]), _ptr(out["scores"]),
        _ptr(out["targets"]), _ptr(out["inside"]), _ptr(out["outside"]), _ptr(out["assign"]), _ptr(out["counts"]),
        _ptr(skip_mask), _stream()), "frcnn_proposal_target_layer")
    return out


def fpn_level_map(rois, k_min, k_max, canonical_scale=224.0, canonical_level=4.0, eps=1e-6):
    """rois (R,5) -> int32 (R,) pyramid level relative to k_min (LevelMapper, torchpoolers.py:39-51)."""
    lib = _hip.load()
    _dev_f32(rois, "rois")
    levels = torch.empty((rois.shape[0],), dtype=torch.int32, device=rois.device)
    _hip.check(lib.frcnn_fpn_level_map(_ptr(rois), rois.shape[0], int(k_min), int(k_max), float(canonical_scale),
                                       float(canonical_level), float(eps), _ptr(levels), _stream()), "frcnn_fpn_level_map")
    return levels


def spatial_mean(x):
    """(R,P,P,C) NHWC -> (R,C): x.mean(3).mean(2) of the NCHW-shaped view."""
    lib = _hip.load()
    _dev_f32(x, "x")
    r, p, _, c = x.shape
    out = torch.empty((r, c), dtype=torch.float32, device=x.device)
    _hip.check(lib.frcnn_spatial_mean_fwd(_ptr(x), _ptr(out), r, p, c, _stream()), "frcnn_spatial_mean_fwd")
    return out


def spatial_mean_bwd(dout, pooled):
    lib = _hip.load()
    _dev_f32(dout, "dout")
    r, c = dout.shape
    dx = torch.empty((r, pooled, pooled, c), dtype=torch.float32, device=dout.device)
    _hip.check(lib.frcnn_spatial_mean_bwd(_ptr(dout), _ptr(dx), r, pooled, c, _stream()), "frcnn_spatial_mean_bwd")
    return dx


# frcnn_sgd_update: elements per workgroup and the 32-byte row of the segment table (include/frcnn_hip.h frcnn_sgd_segment)
SGD_CHUNK = 4096


def sgd_segment_dtype():
    import numpy as np
    return np.dtype([('param', '<u8'), ('offset', '<i8'), ('count', '<i8'), ('lr', '<f4'), ('weight_decay', '<f4')])


def sgd_tables(param_ptrs, offsets, counts, lrs, weight_decays):
    """Host tables of ``sgd_update``: the segment table (one ``sgd_segment_dtype`` row per parameter) and the chunk table
    (int32 (num_chunks, 2): segment, chunk index; ceil(count / SGD_CHUNK) rows per segment)."""
    import numpy as np
    seg = np.zeros(len(param_ptrs), dtype=sgd_segment_dtype())
    seg['param'], seg['offset'], seg['count'] = param_ptrs, offsets, counts
    seg['lr'], seg['weight_decay'] = lrs, weight_decays
    per = (seg['count'] + SGD_CHUNK - 1) // SGD_CHUNK
    chunks = np.empty((int(per.sum()), 2), dtype=np.int32)
    chunks[:, 0] = np.repeat(np.arange(len(seg), dtype=np.int32), per)
    chunks[:, 1] = np.concatenate([np.arange(n, dtype=np.int32) for n in per] or [np.zeros(0, np.int32)])
    return seg, chunks


def sgd_update(grad_flat, momentum_flat, segments_host, segments_dev, chunks_dev, momentum, clip=0.0, zero_grads=False):
    """The solver's weight update for all parameters in one launch (frcnn_sgd_update; lib/model/train_val.py:207-208,
    379-382): per element g = clamp(g, -clip, clip); d = g + wd * p; b = b * momentum + d; p = p - lr * b; g = 0 when
    ``zero_grads``.  ``grad_flat`` / ``momentum_flat``: flat fp32 device buffers of one layout; ``segments_host``: the numpy
    segment table of ``sgd_tables``, ``segments_dev`` its copy on the device as uint8 (the caller keeps them equal: the
    arguments are checked on the host copy), ``chunks_dev``: the chunk table on the device, int32 (num_chunks, 2).
    ``clip`` <= 0 or inf: no clip.  The parameters are written through the pointers in the table: the caller bumps their
    version counters."""
    lib = _hip.load()
    _dev_f32(grad_flat, "sgd_update: grad_flat")
    _dev_f32(momentum_flat, "sgd_update: momentum_flat")
    if grad_flat.dim() != 1 or momentum_flat.shape != grad_flat.shape or momentum_flat.device != grad_flat.device:
        raise _hip.HipError("sgd_update: grad_flat and momentum_flat must be flat buffers of one size on one device")
    if segments_host.dtype != sgd_segment_dtype() or segments_host.ndim != 1 or not segments_host.flags['C_CONTIGUOUS']:
        raise _hip.HipError("sgd_update: segments_host must be a contiguous 1-d array of sgd_segment_dtype()")
    num = int(segments_host.shape[0])
    for t, name, dtype, count in ((segments_dev, "segments_dev", torch.uint8, num * 32),
                                  (chunks_dev, "chunks_dev", torch.int32, None)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != grad_flat.device:
            raise _hip.HipError("sgd_update: %s must be a tensor on the MI355X (got %s); this package has no CPU path"
                                % (name, getattr(t, "device", type(t))))
        if t.dtype != dtype or not t.is_contiguous() or (count is not None and t.numel() != count):
            raise _hip.HipError("sgd_update: %s must be contiguous %s%s" % (name, dtype, "" if count is None else " of %d bytes" % count))
    if chunks_dev.dim() != 2 or chunks_dev.shape[1] != 2:
        raise _hip.HipError("sgd_update: chunks_dev must have shape (num_chunks, 2), got %s" % (tuple(chunks_dev.shape),))
    _hip.check(lib.frcnn_sgd_update(_ptr(grad_flat), _ptr(momentum_flat), grad_flat.numel(),
                                    _ptr(segments_dev) if num else None, segments_host.ctypes.data if num else None, num,
                                    _ptr(chunks_dev) if chunks_dev.numel() else None, int(chunks_dev.shape[0]),
                                    float(momentum), float(clip), int(bool(zero_grads)), _stream()), "frcnn_sgd_update")


# frcnn_draw_*: the draw list's row layout and kinds, the two BEV colourings (include/frcnn_hip.h FRCNN_DRAW_*)
DRAW_ROW_INTS = 12
DRAW_SKIP, DRAW_RECT, DRAW_FOOTPRINT = 0, 1, 2
DRAW_BEV_FORMS = {'waymo': 0, 'kitti': 1}
DRAW_MAX_OUT = 4096


def _draw_dev(who, t, name, dtype, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _hip.HipError("%s: %s must be a tensor on the MI355X (got %s); this package has no CPU path"
                            % (who, name, getattr(t, "device", type(t))))
    if t.dtype != dtype or not t.is_contiguous():
        raise _hip.HipError("%s: %s must be contiguous %s (got %s)" % (who, name, dtype, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _hip.HipError("%s: %s has shape %s, expected %s" % (who, name, tuple(t.shape), tuple(shape)))
    return t


def _draw_out(who, out, name, dtype, shape, device):
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    return _draw_dev(who, out, name, dtype, shape)


def canvas_from_image_blob(blob, out=None):
    """The image blob back to a picture (frcnn_canvas_from_image_blob; lib/datasets/waymo_imdb.py:200-204): ``blob``
    (1, H, W, 3) fp32 -> (H, W, 3) uint8, ``blob * cfg.PIXEL_STDDEVS + cfg.PIXEL_MEANS`` in float64, channels in
    ``cfg.PIXEL_ARRANGE_BGR`` order, truncated toward zero, saturated to [0, 255], NaN -> 0."""
    from .model.config import cfg
    who = "canvas_from_image_blob"
    _dev_f32(blob, who + ": blob")
    if blob.dim() != 4 or blob.shape[0] != 1 or blob.shape[3] != 3:
        raise _hip.HipError("%s: blob must be (1, H, W, 3), got %s" % (who, tuple(blob.shape)))
    h, w = int(blob.shape[1]), int(blob.shape[2])
    out = _draw_out(who, out, "out", torch.uint8, (h, w, 3), blob.device)
    stds = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(cfg.PIXEL_STDDEVS, np.float64).reshape(-1)])
    means = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(cfg.PIXEL_MEANS, np.float64).reshape(-1)])
    arrange = (ctypes.c_int * 3)(*[int(v) for v in cfg.PIXEL_ARRANGE_BGR])
    _hip.check(_hip.load().frcnn_canvas_from_image_blob(_ptr(blob), h, w, stds, means, arrange, _ptr(out), _stream()),
               "frcnn_canvas_from_image_blob")
    return out


def canvas_from_bev_blob(blob, form, num_slices=None, out=None, ws=None):
    """The BEV voxel grid as a picture (frcnn_canvas_from_bev_blob): ``blob`` (1, Ny, Nx, C) fp32 -> (Ny, Nx, 3) uint8,
    ``form`` 'waymo' (lib/datasets/waymo_lidb.py:240-261) or 'kitti' (kitti_lidb.py:289-297, also CADC's).  The blob is
    only read.  ``num_slices`` defaults to cfg.LIDAR.NUM_SLICES."""
    from .model.config import cfg
    who = "canvas_from_bev_blob"
    _dev_f32(blob, who + ": blob")
    if blob.dim() != 4 or blob.shape[0] != 1:
        raise _hip.HipError("%s: blob must be (1, Ny, Nx, C), got %s" % (who, tuple(blob.shape)))
    if form not in DRAW_BEV_FORMS:
        raise _hip.HipError("%s: form %r, one of %s" % (who, form, sorted(DRAW_BEV_FORMS)))
    ny, nx, c = (int(v) for v in blob.shape[1:])
    slices = int(cfg.LIDAR.NUM_SLICES if num_slices is None else num_slices)
    out = _draw_out(who, out, "out", torch.uint8, (ny, nx, 3), blob.device)
    lib = _hip.load()
    ws_bytes = lib.frcnn_canvas_from_bev_blob_ws_bytes()
    ws = _given_workspace(who, ws, ws_bytes, blob.device)
    _hip.check(lib.frcnn_canvas_from_bev_blob(_ptr(blob), ny, nx, c, slices, DRAW_BEV_FORMS[form], _ptr(out), _ptr(ws),
                                              ws.numel() * ws.element_size(), _stream()), "frcnn_canvas_from_bev_blob")
    return out


def canvas_bev_workspace(device):
    """A workspace for ``canvas_from_bev_blob`` (the per-workgroup extrema and the three factors)."""
    return torch.empty(int(_hip.load().frcnn_canvas_from_bev_blob_ws_bytes()), dtype=torch.uint8, device=device)


def draw_plan_capacity(num_classes, max_out, num_gt):
    return (int(num_classes) - 1) * int(max_out) + int(num_gt)


def draw_plan(dets, counts, canvas_hw, lidar, key=None, limiter0=15, limiter_resets=None, gt=None, gt_labels=None,
              rows=None):
    """A frame's device record -> its draw list in painter's order (frcnn_draw_plan; include/frcnn_hip.h has the rules).
    ``dets`` (K, max_out, E) fp32 and ``counts`` (K,) int32 as ``detect_frame_device`` returns them; ``key``: None or
    ``(first column, column count)`` of the uncertainty that orders a class's detections; ``gt`` (G, 4 or 7) fp32 and
    ``gt_labels`` (G,) int32 device tensors or None; ``limiter_resets`` defaults to the reference's rule for the frame
    kind (image: resets, LiDAR: carries).  Returns int32 (capacity, DRAW_ROW_INTS), capacity = (K-1) * max_out + G."""
    who = "draw_plan"
    _dev_f32(dets, who + ": dets")
    if dets.dim() != 3:
        raise _hip.HipError("%s: dets must be (K, max_out, E), got %s" % (who, tuple(dets.shape)))
    k, max_out, elem = (int(v) for v in dets.shape)
    _draw_dev(who, counts, "counts", torch.int32, (k,))
    num_gt = 0
    if gt is not None and gt.numel():
        _draw_dev(who, gt, "gt", torch.float32)
        if gt.dim() != 2 or gt.shape[1] != (7 if lidar else 4):
            raise _hip.HipError("%s: gt must be (G, %d), got %s" % (who, 7 if lidar else 4, tuple(gt.shape)))
        num_gt = int(gt.shape[0])
        _draw_dev(who, gt_labels, "gt_labels", torch.int32, (num_gt,))
    capacity = draw_plan_capacity(k, max_out, num_gt)
    rows = _draw_out(who, rows, "rows", torch.int32, (capacity, DRAW_ROW_INTS), dets.device)
    key_col, key_cols = (0, 0) if key is None else (int(key[0]), int(key[1]))
    if limiter_resets is None:
        limiter_resets = not lidar
    if capacity == 0:
        return rows
    _hip.check(_hip.load().frcnn_draw_plan(_ptr(dets), _ptr(counts), k, max_out, elem, int(bool(lidar)), key_col, key_cols,
                                           int(limiter0), int(bool(limiter_resets)), _ptr(gt) if num_gt else None,
                                           _ptr(gt_labels) if num_gt else None, num_gt, int(canvas_hw[0]),
                                           int(canvas_hw[1]), _ptr(rows), capacity, _stream()), "frcnn_draw_plan")
    return rows


def draw_boxes(canvas, rows, owner=None):
    """Paint a draw list onto ``canvas`` (H, W, 3) uint8 in place, in exact painter's order (frcnn_draw_scatter +
    frcnn_draw_compose): row i beats every row before it wherever their outlines cross, whatever the scheduling.
    ``rows``: int32 (N, DRAW_ROW_INTS); ``owner``: optional (H, W) int32 scratch plane.  Returns ``canvas``."""
    who = "draw_boxes"
    _draw_dev(who, canvas, "canvas", torch.uint8)
    if canvas.dim() != 3 or canvas.shape[2] != 3:
        raise _hip.HipError("%s: canvas must be (H, W, 3), got %s" % (who, tuple(canvas.shape)))
    h, w = int(canvas.shape[0]), int(canvas.shape[1])
    _draw_dev(who, rows, "rows", torch.int32)
    if rows.dim() != 2 or rows.shape[1] != DRAW_ROW_INTS:
        raise _hip.HipError("%s: rows must be (N, %d), got %s" % (who, DRAW_ROW_INTS, tuple(rows.shape)))
    n = int(rows.shape[0])
    owner = _draw_out(who, owner, "owner", torch.int32, (h, w), canvas.device)
    lib = _hip.load()
    _hip.check(lib.frcnn_draw_scatter(_ptr(rows) if n else None, n, _ptr(owner), h, w, _stream()), "frcnn_draw_scatter")
    _hip.check(lib.frcnn_draw_compose(_ptr(rows) if n else None, n, _ptr(owner), _ptr(canvas), h, w, _stream()),
               "frcnn_draw_compose")
    return canvas
