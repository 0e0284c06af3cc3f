"""Glue between ``torch.nn`` parameter containers and the HIP kernels.

``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.Linear`` objects are kept ONLY as owners of parameters so that
``state_dict()`` keys, ``named_parameters()`` and ``.requires_grad`` behave exactly like the reference's
modules (lib/model/train_val.py:188-206 builds its optimizer groups from them).  Their torch ``forward``
is never used on the hot path: ``conv_bn_act`` reads the parameters, lays the filter out as KRSC with the
input channels padded to a multiple of 4, folds an eval-mode BatchNorm into a per-channel scale/shift and
launches ``frcnn_conv2d_fwd``.  Prepared tensors are cached on the module and keyed by the parameters'
version counters, so ``load_state_dict`` / optimizer steps invalidate them automatically.

Activations between modules are NHWC ``(N, H, W, C)`` contiguous tensors.
"""
import torch
import torch.nn as nn

from .. import ops
from ..model.config import cfg


def pad4(c):
    return (c + 3) // 4 * 4


def stable_store(holder, name, key, fresh, refresh=None):
    """Cache ``fresh`` (a tuple of tensors / None) under ``holder.__dict__[name]`` keyed by ``key`` - INTO THE STORAGE OF THE
    PREVIOUS ENTRY when there is one of the same shapes.  Weight-derived tensors (KRSC filters, folded BatchNorm terms,
    transposed and Winograd filters, fused head filters) therefore keep their device addresses across optimizer steps, which
    is what a captured training graph (model/train_graph.py) reads.  ``refresh``: zero-argument callable that re-derives
    this entry from the live parameters (``refresh_derived_weights`` calls it after an optimizer step, since a replayed
    graph runs no Python that would notice the parameters' new version)."""
    d = holder.__dict__
    old = d.get(name)
    value = fresh
    if old is not None and len(old[1]) == len(fresh) and all(
            (o is None) == (f is None) and (o is None or (o.shape == f.shape and o.device == f.device))
            for o, f in zip(old[1], fresh)):
        with torch.no_grad():
            for o, f in zip(old[1], fresh):
                if o is not None and o.data_ptr() != f.data_ptr():
                    o.copy_(f)
        value = old[1]
    d[name] = (key, value)
    if refresh is not None:
        d[name + '_refresh'] = refresh
    return value


# derived entries that read other derived entries (the KRSC filter) come second
_REFRESH_ORDER = ('_frcnn_prepared', '_frcnn_perm', '_fused_cache', '_heads_cache', '_frcnn_wt', '_frcnn_winograd',
                  '_frcnn_dgrad_winograd', '_bf16')


def refresh_derived_weights(net):
    """Re-derive every cached weight-dependent tensor of ``net`` in place (see ``stable_store``).  Returns the number of
    entries visited."""
    holders = [net] + [m for m in net.modules() if m is not net]
    for h in list(holders):
        holders += [v for k, v in h.__dict__.items() if k.endswith('_holder')]
    todo = []
    for h in holders:
        for k, fn in list(h.__dict__.items()):
            if k.endswith('_refresh') and callable(fn):
                rank = next((i for i, tag in enumerate(_REFRESH_ORDER) if tag in k), len(_REFRESH_ORDER))
                todo.append((rank, fn))
    for _, fn in sorted(todo, key=lambda t: t[0]):
        fn()
    return len(todo)


def _versions(*tensors):
    return tuple((t._version, t.data_ptr()) if t is not None else None for t in tensors)


def prepared_conv(conv, bn=None, use_bn=True):
    """Returns (w_krsc, scale, shift) device tensors for ``conv`` (+ eval-mode ``bn`` folded in)."""
    bn = bn if (bn is not None and use_bn) else None
    key_tensors = [conv.weight, conv.bias]
    if bn is not None:
        key_tensors += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    # the batch-norm training kernel updates the running statistics through raw pointers (no torch version bump):
    # autograd_ops._BnTrainFn counts those updates on the module instead
    stats_version = bn.__dict__.get('_frcnn_stats_version', 0) if bn is not None else 0
    key = (_versions(*key_tensors), str(conv.weight.device), stats_version)
    cache = conv.__dict__.get('_frcnn_prepared')
    if cache is not None and cache[0] == key:
        return cache[1]
    with torch.no_grad():
        w = conv.weight.detach()
        k, c, r, s = w.shape
        cp = pad4(c)
        w_krsc = torch.zeros((k, r, s, cp), dtype=torch.float32, device=w.device)
        w_krsc[..., :c] = w.permute(0, 2, 3, 1)
        scale = shift = None
        if bn is not None:
            # F.batch_norm(eval): (x - mean) / sqrt(var + eps) * weight + bias  ->  x*scale + shift
            scale = (bn.weight.detach() / torch.sqrt(bn.running_var.detach() + bn.eps)).contiguous()
            shift = (bn.bias.detach() - bn.running_mean.detach() * scale).contiguous()
            if conv.bias is not None:
                shift = (shift + conv.bias.detach() * scale).contiguous()
        elif conv.bias is not None:
            shift = conv.bias.detach().contiguous()
    return stable_store(conv, '_frcnn_prepared', key, (w_krsc.contiguous(), scale, shift),
                        refresh=lambda: prepared_conv(conv, bn, use_bn))


def prepared_depthwise(conv, bn):
    """(w_rsc (3,3,C), scale (C,), shift (C,)) of a depthwise 3x3 ``conv`` (groups == C, no bias) with its eval-mode ``bn``
    folded in, for ``ops.depthwise_conv3x3_nhwc``.  Cached like ``prepared_conv``: storage-stable (a captured frame reads
    the tensors by address) with a refresh hook (``refresh_derived_weights`` finds it after a weight change)."""
    c = conv.weight.shape[0]
    if (conv.groups != c or tuple(conv.weight.shape) != (c, 1, 3, 3) or conv.bias is not None
            or tuple(conv.padding) != (1, 1) or tuple(conv.dilation) != (1, 1) or tuple(conv.stride) not in ((1, 1), (2, 2))):
        raise NotImplementedError("prepared_depthwise: not a bias-free 3x3 / pad 1 / stride 1|2 depthwise convolution: %r" % (conv,))
    stats_version = bn.__dict__.get('_frcnn_stats_version', 0)
    key = (_versions(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var), str(conv.weight.device), stats_version)
    cache = conv.__dict__.get('_frcnn_prepared_dw')
    if cache is not None and cache[0] == key:
        return cache[1]
    with torch.no_grad():
        w_rsc = conv.weight.detach().reshape(c, 3, 3).permute(1, 2, 0).contiguous()
        scale = (bn.weight.detach() / torch.sqrt(bn.running_var.detach() + bn.eps)).contiguous()
        shift = (bn.bias.detach() - bn.running_mean.detach() * scale).contiguous()
    return stable_store(conv, '_frcnn_prepared_dw', key, (w_rsc, scale, shift), refresh=lambda: prepared_depthwise(conv, bn))


def prepared_conv_concat(owner, cache_name, parts):
    """Several convolutions that read the SAME input with the same geometry as ONE: ``parts`` = [(conv, bn, use_bn), ...] ->
    (w_krsc (K1 + K2 + .., R, S, C), scale (K,), shift (K,)) with the folded BatchNorm terms concatenated (1 / 0 where a
    part has none).  Cached on ``owner`` in storage-stable tensors like every derived weight (captured frames read them by
    address); the entry's name must contain '_fused_cache' so that refresh_derived_weights visits it after the parts."""
    prepared = [prepared_conv(c, b, u) for c, b, u in parts]
    key = tuple((t.data_ptr(), t._version) if t is not None else None for p in prepared for t in p)
    cache = owner.__dict__.get(cache_name)
    if cache is not None and cache[0] == key:
        return cache[1]
    with torch.no_grad():
        w = torch.cat([p[0] for p in prepared], 0).contiguous()
        scale = torch.cat([p[1] if p[1] is not None else torch.ones(p[0].shape[0], device=w.device) for p in prepared]).contiguous()
        shift = torch.cat([p[2] if p[2] is not None else torch.zeros(p[0].shape[0], device=w.device) for p in prepared]).contiguous()
    return stable_store(owner, cache_name, key, (w, scale, shift), refresh=lambda: prepared_conv_concat(owner, cache_name, parts))


def conv_bn_act(x, conv, bn=None, relu=False, residual=None, use_bn=True, winograd_residual=False):
    """NHWC in, NHWC out: act(bn(conv(x)) + residual) on the matrix cores (fp32; bf16 operands under cfg.TEST.CONV_BF16).
    ``winograd_residual``: see ``conv_forward``."""
    if bn is not None and use_bn and bn.training:
        raise NotImplementedError("BatchNorm in training mode (batch statistics) is not on the HIP path yet")
    w, scale, shift = prepared_conv(conv, bn, use_bn)
    if x.shape[-1] != w.shape[-1]:
        x = ops.pad_channels(x, w.shape[-1])
    stride = conv.stride[0] if isinstance(conv.stride, (tuple, list)) else conv.stride
    pad = conv.padding[0] if isinstance(conv.padding, (tuple, list)) else conv.padding
    return conv_forward(x, w, scale, shift, residual, conv, stride=stride, pad=pad, relu=relu, winograd_of=conv,
                        winograd_residual=winograd_residual)


# The mode of the Network.forward in progress ('TRAIN' / 'TEST'): frozen blocks of a training net are in eval() too, so
# the modules' own state does not tell an inference frame from a training step.
_NET_MODE = None


def set_net_mode(mode):
    global _NET_MODE
    _NET_MODE = mode


def conv_bf16_eligible(c, k, r, s, stride, pad, strided_out=False):
    """Can ``ops.conv2d_nhwc_bf16`` run a convolution of this geometry?  (C % 32 == 0: a 32-wide reduction step lies inside
    one filter tap; any k >= 1; no strided output.)"""
    return (c > 0 and c % 32 == 0 and k >= 1 and r >= 1 and s >= 1 and stride >= 1 and pad >= 0 and not strided_out)


def conv_bf16_train_eligible(c, k, r, s, stride, pad, has_gradient=True):
    """THE rule of cfg.TRAIN.CONV_BF16 for one convolution of a ``_BottleneckFn`` / ``_ConvFn`` (``conv_bn_act_train``) node:
    it has a trainable filter or a gradient passes through it (``has_gradient``), and C % 32 == 0 and K % 32 == 0 - then its
    forward, its data gradient and its filter gradient all multiply bf16-rounded operands.  A convolution is eligible as a
    whole or not at all; the one exception inside an eligible convolution is the strided 1x1 DATA gradient, which writes a
    scattered output the bf16 kernel does not have and stays fp32 (``conv_bf16_train_dgrad_fp32``).  Everything else - the
    stem, the RPN's patch convolutions, the fused heads, ``linear_train``, the MobileNet and VGG16 nodes, any C or K that is
    no multiple of 32 - never asks.  No per-shape exclusions (profiles/conv_bf16_train.md)."""
    return bool(has_gradient and c > 0 and c % 32 == 0 and k > 0 and k % 32 == 0 and r >= 1 and s >= 1 and stride >= 1 and pad >= 0)


def conv_bf16_train_dgrad_fp32(r, s, stride):
    """The stated exception of ``conv_bf16_train_eligible``: the strided 1x1 data gradient stays fp32."""
    return stride > 1 and r == 1 and s == 1


def conv_bf16_train_wanted(w_krsc, stride, pad, has_gradient):
    """cfg.TRAIN.CONV_BF16, a TRAIN-mode forward and an eligible convolution (``conv_bf16_train_eligible``).  Asked once, in the
    node's forward; its backward follows that answer."""
    if not cfg.TRAIN.get('CONV_BF16', False) or _NET_MODE != 'TRAIN':
        return False
    k, r, s, c = w_krsc.shape
    return conv_bf16_train_eligible(c, k, r, s, stride, pad, has_gradient)


def conv_bf16_wanted(x, w_krsc, stride, pad):
    """cfg.TEST.CONV_BF16, a TEST-mode forward, no gradient wanted and an eligible layer."""
    if not cfg.TEST.get('CONV_BF16', False) or _NET_MODE != 'TEST' or (torch.is_grad_enabled() and x.requires_grad):
        return False
    k, r, s, c = w_krsc.shape
    return x.shape[-1] == c and conv_bf16_eligible(c, k, r, s, stride, pad)


def conv_split_bf16_wanted(x, w_krsc, stride, pad):
    """cfg.TEST.CONV_SPLIT_BF16, a TEST-mode forward, no gradient wanted, C % 32 == 0 and the library's rule
    (``ops.conv_split_bf16_wanted``: the large GEMMs; no while a forced tile, ``set_conv_algo``, the staging mode or
    ``frcnn_conv2d_split_bf16_enable(0)`` pins the fp32 kernels; an imported plan table does not) says yes."""
    if not cfg.TEST.get('CONV_SPLIT_BF16', True) or _NET_MODE != 'TEST' or (torch.is_grad_enabled() and x.requires_grad):
        return False
    k, r, s, c = w_krsc.shape
    if x.dim() != 4 or x.shape[-1] != c or not conv_bf16_eligible(c, k, r, s, stride, pad):
        return False
    n, h, w, _ = x.shape
    return ops.conv_split_bf16_wanted(n, h, w, c, k, r, s, stride, pad)


def _bf16_entry(holder, name, w_krsc, pack=None):
    """``w_krsc`` packed for ``ops.conv2d_nhwc_bf16`` (``pack``: another packer - ``ops.conv2d_pack_bf16x3`` for the split
    form, under a name of its own), cached on ``holder`` next to the fp32 filter it was made from and
    re-packed IN PLACE when that filter changed (also the entry's refresh hook, after the filter's own).  A cache miss
    inside a stream capture would launch the packing into the graph and pin a graph-pool tensor on the module: it raises
    instead (run one eager frame first)."""
    cache = holder.__dict__.get(name)
    key = (w_krsc.data_ptr(), w_krsc._version, tuple(w_krsc.shape))
    if cache is not None and cache[0] == key:
        return cache[1][0]
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("bf16 filter of a %s layer is not prepared: run an eager frame before capturing" % (tuple(w_krsc.shape),))
    packed = (pack or ops.conv2d_pack_bf16)(w_krsc)
    return stable_store(holder, name, key, (packed,), refresh=lambda: _bf16_entry(holder, name, w_krsc, pack))[0]


def conv_forward(x, w_krsc, scale, shift, residual, holder, stride=1, pad=0, relu=False, winograd_of=None,
                 cache_name='_frcnn_bf16', winograd_residual=False):
    """The one forward convolution of the inference call sites.  With cfg.TEST.CONV_BF16 in a TEST-mode forward an eligible
    layer (``conv_bf16_eligible``) runs ``ops.conv2d_nhwc_bf16`` on its packed filter, cached on ``holder`` under
    ``cache_name``; after it, with cfg.TEST.CONV_SPLIT_BF16 (default on), a layer the library's rule selects runs the
    fp32-accurate ``ops.conv2d_nhwc_bf16x3`` (filter cached under ``cache_name + 'x3'``); every other call is ``ops.conv2d_nhwc`` exactly as without the switch (``winograd_of``: the module whose
    pre-transformed Winograd filter a residual-free call may read).  ``winograd_residual`` (default off; only
    ``nets.resnet.BasicBlock`` passes it): a call WITH a residual whose fp32 route is ``ops.conv2d_nhwc_winograd_res``; the
    bf16 switches come first as everywhere, with the residual in their own epilogue."""
    if conv_bf16_wanted(x, w_krsc, stride, pad):
        return ops.conv2d_nhwc_bf16(x, _bf16_entry(holder, cache_name, w_krsc), scale, shift, residual, stride=stride, pad=pad,
                                    relu=relu)
    if conv_split_bf16_wanted(x, w_krsc, stride, pad):
        return ops.conv2d_nhwc_bf16x3(x, _bf16_entry(holder, cache_name + 'x3', w_krsc, ops.conv2d_pack_bf16x3), scale, shift,
                                      residual, stride=stride, pad=pad, relu=relu)
    u = None
    if winograd_residual:
        # BasicBlock's closing convolution: planned as the residual-free call of its shape, the residual goes into the
        # Winograd output transform where that plan is Winograd (ops.conv2d_nhwc_winograd_res); U from the same cache
        k, r, s, c = w_krsc.shape
        if residual is None or not ops.winograd_eligible(k, r, s, c, stride, pad):
            raise ValueError("conv_forward: winograd_residual needs a residual and a 3x3 / stride 1 / pad 1 layer with "
                             "C % 4 == 0 and K % 4 == 0")
        if winograd_of is not None:
            u = _winograd_filter(winograd_of, w_krsc, tuple(x.shape[:3]), stride, pad)
        return ops.conv2d_nhwc_winograd_res(x, w_krsc, residual, scale, shift, relu=relu, w_winograd=u)
    if winograd_of is not None and residual is None:
        n, h, wd, c = x.shape
        u = _winograd_filter(winograd_of, w_krsc, (n, h, wd), stride, pad)
    return ops.conv2d_nhwc(x, w_krsc, scale, shift, residual, stride=stride, pad=pad, relu=relu, w_winograd=u)


def _winograd_filter(conv, w_krsc, nhw, stride, pad):
    """The Winograd-transformed filter U of an eligible 3x3 layer, cached next to the KRSC filter it was made from
    (``prepared_conv`` makes a new one per parameter version), so the inference path does not redo the transform per frame.
    U (1.78x the filter) is only built for a layer and shape whose plan reads it (``ops.winograd_filter_wanted``: a cached
    Winograd plan, forced Winograd, or a shape the autotuner is about to time); under set_conv_algo(1) or an implicit-GEMM
    plan nothing is transformed.  Once built it is kept for the lifetime of the module (a captured graph may have baked
    its address in).  A cache miss inside a stream capture would launch the transform
    into the graph and pin a graph-pool tensor on the module: it raises instead (run one eager frame first)."""
    k, r, s, c = w_krsc.shape
    n, h, w = nhw
    if not ops.winograd_filter_wanted(n, h, w, c, k, r, s, stride, pad):
        # this SHAPE's plan does not read U.  An entry made for another shape of the same layer stays, with its refresh
        # hook: a captured graph of that shape (FrameRunner / TrainStepRunner) reads U by device address, so it must
        # neither be freed nor fall out of refresh_derived_weights (two frame sizes whose plans differ, e.g. KITTI).
        return None
    return _winograd_entry(conv, w_krsc)


def _winograd_entry(conv, w_krsc):
    """U of ``conv`` for the current contents of ``w_krsc``: the cached tensor, re-derived IN PLACE when the filter changed.
    Also the entry's refresh hook - which therefore does not depend on the plan tables or the algorithm switch at the time
    an optimizer step / load_state_dict is noticed."""
    k, _, _, c = w_krsc.shape
    cache = conv.__dict__.get('_frcnn_winograd')
    key = (w_krsc.data_ptr(), w_krsc._version)
    if cache is not None and cache[0] == key:
        return cache[1][0]
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("Winograd filter of a %dx%dx3x3 layer is not prepared: run an eager frame before capturing" % (k, c))
    return stable_store(conv, '_frcnn_winograd', key, (ops.winograd_filter(w_krsc),),
                        refresh=lambda: _winograd_entry(conv, w_krsc))[0]


def to_nhwc(t):
    """NCHW-shaped tensor (any strides) -> contiguous NHWC tensor; free for channels_last inputs."""
    v = t.permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


def to_nchw_view(t):
    """NHWC contiguous tensor -> NCHW-shaped view (channels_last strides), no copy."""
    return t.permute(0, 3, 1, 2)


class MaxPool3x3s2(nn.Module):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1) of the stem (lib/nets/resnet.py:156), NHWC."""

    def forward(self, x):
        return ops.maxpool3x3s2_nhwc(x)
