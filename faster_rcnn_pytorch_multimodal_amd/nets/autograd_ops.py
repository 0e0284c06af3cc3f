"""Autograd nodes of the training path (``Network.train_step`` -> ``loss.backward()``,
lib/model/train_val.py:458): each node's forward AND backward are libfrcnn_hip.so launches
(``frcnn_conv2d_fwd / _bwd_data / _bwd_weight``, ``frcnn_act_bwd``, ``frcnn_upsample_bilinear_*``,
``frcnn_roi_align_fwd / _bwd``, ``frcnn_rpn_loss``, ``frcnn_det_loss``, and for MobileNet-v1 ``frcnn_dwconv3x3_fwd /
_bwd_data / _bwd_weight`` and ``frcnn_act_bwd_cap``, for VGG16 ``frcnn_maxpool2x2s2_fwd / _bwd`` and
``frcnn_dropout_fwd / _bwd``).  torch.autograd only orders the nodes
and owns the ``.grad`` buffers; gradient accumulation inside a residual block is fused into the data-gradient
kernel's epilogue (``add=``), so a Bottleneck is ONE node.

BatchNorm of the image detector is frozen (lib/nets/imagenet.py:110-116): a per-channel scale/shift of the
convolution output that receives no gradient.  The LiDAR backbone trains its BatchNorm layers with batch statistics
(lib/nets/lidarnet.py:110,152-175): ``_BnTrainFn`` = ``frcnn_bn_train_fwd / _bwd``.  Activations are NHWC; parameters keep the reference's layouts
(Conv2d (K,C,R,S), Linear (out,in)) and are re-laid out as KRSC through ``hip_modules.prepared_conv`` caches.
"""
import collections
import contextlib
import os

import torch

from .. import ops
from .hip_modules import (_bf16_entry, _winograd_filter, conv_bf16_train_dgrad_fp32, conv_bf16_train_wanted, pad4, prepared_conv,
                          prepared_depthwise, stable_store)


# How one pass launches its filter gradients.  They are off the critical path of backward (only the data gradient feeds the next
# node), so a pass may accumulate them into ``param.grad`` itself instead of returning them to autograd;
# ``join_weight_grads()`` (called by Network.backward before clipping / the optimizer) then completes them.
#   accumulate    False: gradients go back to autograd, the other fields are not read.  True: this package's own launches add
#                 into ``param.grad`` (a captured step: autograd's AccumulateGrad nodes run on the parameter's creation stream,
#                 outside the capture).  Measured on the eager FPN step (round 1): no gain, the step is bound by GPU throughput.
#   side_stream   True: on a side stream next to the data-gradient chain - a captured step is a forked graph.  False: in line on
#                 the step's own stream - ONE chain of kernel nodes, the form the runtime overlaps when several replays are in
#                 flight (model/train_graph.TrainPipeline: two replays of a forked graph were measured not to overlap at all;
#                 train_graph.inline_graphs_supported and the replay check guard the runtime fault this form once hit).
#   grouped       repeated layers of identical shape - the 22 equal Bottlenecks of layer3 - are collected per shape and launched
#                 TOGETHER (ops.conv2d_bwd_weight_acc_grouped): one launch pair per shape instead of a pixel-split launch + a
#                 slab reduction per layer.  A group is flushed when it is full, when its shape has not come up for _STALE calls
#                 (its stage's backward is over), and at join_weight_grads().  The grouped launches run AFTER their stage's
#                 data-gradient chain instead of next to it: with the register-staged kernel they lost (15.3-15.4 against
#                 15.0-15.2 ms per replayed step, round 3); with conv_wgrad_dma_f32, which adds into param.grad itself, they win
#                 (14.7 -> 14.3 ms, round 5).
#   bn_stat_sink  {id(BatchNorm module): [mean buffer, variance buffer, used]} while a step with DEFERRED running statistics is
#                 captured (model/train_graph.TrainStepRunner(defer_bn_stats=True)), else None: see _BnTrainFn.forward
WgradSchedule = collections.namedtuple('WgradSchedule', 'accumulate side_stream grouped bn_stat_sink')
EAGER_SCHEDULE = WgradSchedule(accumulate=False, side_stream=False, grouped=False, bn_stat_sink=None)
SCHEDULE = EAGER_SCHEDULE       # a plain module global: autograd's backward thread has to see it too


@contextlib.contextmanager
def wgrad_schedule(schedule):
    """Install ``schedule`` for the passes run inside; the previous one is back on exit, also when the body raises."""
    global SCHEDULE
    prev, SCHEDULE = SCHEDULE, schedule
    try:
        yield schedule
    finally:
        SCHEDULE = prev


# Process-wide A/B switches (tools set them before anything is captured).
# Side streams per device.  Every gradient buffer is pinned to ONE of them (first come, round robin): launches that accumulate into
# the same buffer - the RPN head applied to five pyramid levels - stay ordered, launches into different buffers may overlap.
WGRAD_SIDE_STREAMS = 1
# captured steps: the BatchNorm backward adds d_gamma / d_beta into param.grad itself (False: temporaries + add_ launches; A/B)
BN_GRADS_IN_KERNEL = os.environ.get('FRCNN_BN_GRADS_IN_KERNEL', '1') != '0'
GROUP_WGRAD_SIZE = 24  # layers per grouped launch (<= ops.WGRAD_MAX_GROUPS): a whole ResNet stage
_SIDE = {}         # device -> side streams
_STREAM_OF = {}    # (device, id of the gradient's owner) -> index
_KEEP = []         # operands of filter-gradient launches, held until the main stream has joined the side streams
_DEFER = {}        # key -> list of (x, d_conv, grad)
_DEFER_AGE = {}    # key -> _wgrad calls since the key last came up
_STALE = 8


def _launch_wgrad(owner, operands, launch):
    """Run ``launch()`` where the installed schedule puts filter gradients: on the side stream ``owner`` is pinned to, ordered
    after the main stream, or in line.  ``owner``: the gradient buffer the launch accumulates into (the parameter when it
    has no in-place buffer), so that every launch into one buffer lands on one stream."""
    device = operands[0].device
    main = stream = torch.cuda.current_stream(device)
    if SCHEDULE.side_stream:
        pool = _SIDE.setdefault(str(device), [])
        want = max(1, int(WGRAD_SIDE_STREAMS))
        while len(pool) < want:
            pool.append(torch.cuda.Stream(device=device))
        pin = _STREAM_OF.setdefault((str(device), id(owner)), len(_STREAM_OF) % want) if want > 1 else 0
        stream = pool[pin % want]
        stream.wait_stream(main)
    with torch.cuda.stream(stream):
        launch()
    # the side stream still reads the operands when this function's caller drops them, and the allocator would hand their
    # blocks to the next main-stream allocation.  Tensor.record_stream covers that in eager mode; inside a stream capture it
    # was observed not to (run-to-run different gradients from the replayed graph), so the operands are simply kept alive
    # until join_weight_grads() has made the main stream wait for the side stream.
    _KEEP.extend(operands)
    if SCHEDULE.side_stream:
        for t in operands:
            t.record_stream(stream)


def _flush_group(key):
    entries = _DEFER.pop(key, [])
    _DEFER_AGE.pop(key, None)
    if not entries:
        return
    xs, ds, grads = [list(col) for col in zip(*entries)]
    r, s, stride, pad = key[2:6]
    if len(entries) == 1:
        launch = lambda: ops.conv2d_bwd_weight_acc(xs[0], ds[0], r, s, grads[0], None, stride=stride, pad=pad)
    else:
        launch = lambda: ops.conv2d_bwd_weight_acc_grouped(xs, ds, r, s, grads, stride=stride, pad=pad)
    _launch_wgrad(grads[0], xs + ds, launch)


def _defer_wgrad(x, d_conv, r, s, stride, pad, grad):
    key = (tuple(x.shape), tuple(d_conv.shape), r, s, stride, pad, tuple(grad.shape), str(x.device))
    for k in list(_DEFER_AGE):
        _DEFER_AGE[k] += 1
    _DEFER.setdefault(key, []).append((x, d_conv, grad))
    _DEFER_AGE[key] = 0
    if len(_DEFER[key]) >= min(GROUP_WGRAD_SIZE, ops.WGRAD_MAX_GROUPS):
        _flush_group(key)
    for k in [k for k, age in _DEFER_AGE.items() if age >= _STALE]:
        _flush_group(k)


def drop_deferred_weight_grads():
    """Forget collected-but-unlaunched filter gradients (a backward pass that raised must not leak its tensors into the
    next step's groups)."""
    _DEFER.clear()
    _DEFER_AGE.clear()


def join_weight_grads(device=None):
    """Main stream waits for every filter-gradient launch issued so far (no-op when none were issued); deferred groups are
    launched first."""
    for k in list(_DEFER):
        if device is None or k[-1] == str(torch.device(device)):
            _flush_group(k)
    for key, pool in _SIDE.items():
        if device is None or key == str(torch.device(device)):
            for side in pool:
                torch.cuda.current_stream(side.device).wait_stream(side)
    _KEEP.clear()


def _accumulate(param, grad):
    if param.grad is None:
        param.grad = grad
    else:
        param.grad.add_(grad)


def _wgrad(x, d_conv, r, s, stride, pad, weight=None, bias=None, mapped=None, bf16=False):
    """Filter (and bias) gradient of one convolution, one list entry per target: the gradients when the schedule returns
    them to autograd, None for each when it accumulates into param.grad.
    Plain case: ``weight`` [, ``bias``] of ONE module (targets in that order), gradients in the parameters' own layout -
    with the gradient buffers in place it is one launch chain that sums the pixel-split slabs, changes the layout and adds
    into param.grad (no temporaries, no permute copy, no add_), and it may join a group.
    Special layouts (the fused head's K-slices, the permuted Linear): ``mapped`` = list of (param, fn), fn maps
    (dw_krsc, db) to that parameter's gradient; never in place, never grouped.
    ``bf16`` (cfg.TRAIN.CONV_BF16, an eligible convolution): the bf16-operand kernel, launched layer by layer - it has no grouped
    form, so the layer skips the grouped deferral."""
    plain = mapped is None
    if plain:
        mapped = [(weight, lambda dwk, dbk: _param_grad_from_krsc(dwk, weight))] if weight is not None else []
        if bias is not None:
            mapped.append((bias, lambda dwk, dbk: dbk))
    want_bias = bias is not None or not plain

    def param_layout_grads():
        bwd_weight = ops.conv2d_bwd_weight_bf16 if bf16 else ops.conv2d_bwd_weight
        dw_krsc, db = bwd_weight(x, d_conv, r, s, stride=stride, pad=pad, want_bias=want_bias)
        return [fn(dw_krsc, db) for _, fn in mapped]

    if not SCHEDULE.accumulate:
        return param_layout_grads()
    in_place = (plain and weight is not None and all(p.grad is not None and p.grad.is_contiguous() for p, _ in mapped)
                and weight.dim() in (2, 4) and weight.numel() == d_conv.shape[-1] * weight.shape[1] * r * s)
    if in_place and bf16:
        _launch_wgrad(weight.grad, [x, d_conv], lambda: ops.conv2d_bwd_weight_acc_bf16(
            x, d_conv, r, s, weight.grad, bias.grad if bias is not None else None, stride=stride, pad=pad))
    elif in_place and SCHEDULE.grouped and bias is None and weight.dim() == 4:
        _defer_wgrad(x, d_conv, r, s, stride, pad, weight.grad)
    elif in_place:
        _launch_wgrad(weight.grad, [x, d_conv], lambda: ops.conv2d_bwd_weight_acc(
            x, d_conv, r, s, weight.grad, bias.grad if bias is not None else None, stride=stride, pad=pad))
    else:
        # a frozen sibling of a mapped set (one bias of a fused head, the permuted Linear's bias) keeps .grad None, as under autograd
        _launch_wgrad(mapped[0][0], [x, d_conv],
                      lambda: [_accumulate(p, g) for (p, _), g in zip(mapped, param_layout_grads()) if p.requires_grad])
    return [None] * len(mapped)


def _transposed_filter(conv_like, w_krsc):
    """Cached (C,R,S,K) flipped filter of the data-gradient convolution, keyed like the forward filter."""
    cache = conv_like.__dict__.get('_frcnn_wt')
    key = (w_krsc.data_ptr(), w_krsc._version, tuple(w_krsc.shape))
    if cache is not None and cache[0] == key:
        return cache[1][0]
    return stable_store(conv_like, '_frcnn_wt', key, (ops.conv2d_transpose_filter(w_krsc),),
                        refresh=lambda: _transposed_filter(conv_like, w_krsc))[0]


def _conv_fwd_bf16(x, prepared, holder, residual, stride, pad, relu):
    """Forward of an eligible convolution under cfg.TRAIN.CONV_BF16: ``ops.conv2d_nhwc_bf16`` on the packed filter, cached on
    ``holder`` like the inference path's (``_bf16_entry``: re-packed in place when the weights change; a miss inside a capture
    raises).  A layer with a Winograd form in fp32 runs as a direct bf16 convolution."""
    w_krsc, scale, shift = prepared
    return ops.conv2d_nhwc_bf16(x, _bf16_entry(holder, '_frcnn_bf16', w_krsc), scale, shift, residual, stride=stride, pad=pad,
                                relu=relu)


def _bwd_data_bf16(d, holder, w_krsc, x_shape, stride=1, pad=0, add=None, act_y=None, act_scale=None):
    """Data gradient of an eligible convolution under cfg.TRAIN.CONV_BF16: the bf16 GEMM on the bf16 pack of the flipped /
    transposed filter (cached next to ``_frcnn_wt`` under the same rules) - except the strided 1x1 form, whose scattered
    output the bf16 kernel does not have: that one stays fp32."""
    w_t = _transposed_filter(holder, w_krsc)
    if conv_bf16_train_dgrad_fp32(w_krsc.shape[1], w_krsc.shape[2], stride):
        return ops.conv2d_bwd_data(d, w_t, x_shape, stride=stride, pad=pad, add=add, act_y=act_y, act_scale=act_scale)
    return ops.conv2d_bwd_data_bf16(d, _bf16_entry(holder, '_frcnn_dgrad_bf16', w_t), x_shape, stride=stride, pad=pad, add=add,
                                    act_y=act_y, act_scale=act_scale)


RELU6_CAP = 6.0                 # nn.ReLU6 of MobileNet-v1 (_SeparablePairFn)
FUSE_ACT_BWD = True             # False: a separate frcnn_act_bwd pass after each data gradient inside a Bottleneck
DGRAD_WINOGRAD_CACHE = True     # False: the data-gradient convolution transforms its filter on every call


def _dgrad_winograd(conv_like, w_t, x_shape, stride, pad):
    """Winograd transform of the data-gradient filter ``w_t`` (C,3,3,K), cached next to it: the weights change once per
    optimizer step, the data gradient runs once per frame.  None when that convolution's plan is not a Winograd plan (see
    hip_modules._winograd_filter for the rules; a miss inside a stream capture raises)."""
    c, r, s, k = w_t.shape
    if not DGRAD_WINOGRAD_CACHE or r != 3 or stride != 1:
        return None
    if not ops.dgrad_winograd_wanted(x_shape, k, r, s, stride, pad):
        return None          # an entry made for another shape stays (captured graphs read it by address), see _winograd_filter
    return _dgrad_winograd_entry(conv_like, w_t)


def _dgrad_winograd_entry(conv_like, w_t):
    """Cached Winograd form of ``w_t``, re-derived in place when ``w_t`` changed; also the entry's refresh hook."""
    c, _, _, k = w_t.shape
    cache = conv_like.__dict__.get('_frcnn_dgrad_winograd')
    key = (w_t.data_ptr(), w_t._version)
    if cache is not None and cache[0] == key:
        return cache[1][0]
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("Winograd data-gradient filter of a %dx%dx3x3 layer is not prepared: run an eager step before capturing"
                           % (k, c))
    return stable_store(conv_like, '_frcnn_dgrad_winograd', key, (ops.winograd_filter(w_t),),
                        refresh=lambda: _dgrad_winograd_entry(conv_like, w_t))[0]


def _param_grad_from_krsc(dw_krsc, param):
    """(K,R,S,Cpad) -> the parameter's own layout ((K,C,R,S) conv, (out,in) linear)."""
    k, r, s, _ = dw_krsc.shape
    if param.dim() == 2:
        return dw_krsc.view(k, -1)[:, :param.shape[1]].contiguous()
    return dw_krsc[..., :param.shape[1]].permute(0, 3, 1, 2).contiguous()


def _stride_pad(conv):
    st = conv.stride[0] if isinstance(conv.stride, (tuple, list)) else conv.stride
    pd = conv.padding[0] if isinstance(conv.padding, (tuple, list)) else conv.padding
    return st, pd


class _ConvFn(torch.autograd.Function):
    """y = act(conv(x, w) * scale + shift [+ residual]) for ONE parameter set (weight [, bias])."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, pack):
        w_krsc, scale, shift, stride, pad, relu, owner = pack[:7]
        # pack[7] (conv_bn_act_train only): the call site is one cfg.TRAIN.CONV_BF16 covers
        ctx.bf16 = len(pack) > 7 and pack[7] and conv_bf16_train_wanted(w_krsc, stride, pad, any(ctx.needs_input_grad[:4]))
        u = None
        if ctx.bf16:
            y = _conv_fwd_bf16(x, (w_krsc, scale, shift), owner, residual, stride, pad, relu)
        else:
            if residual is None and w_krsc.shape[1] == 3 and isinstance(owner, torch.nn.Module):
                u = _winograd_filter(owner, w_krsc, tuple(x.shape[:3]), stride, pad)
            y = ops.conv2d_nhwc(x, w_krsc, scale, shift, residual, stride=stride, pad=pad, relu=relu, w_winograd=u)
        ctx.pack = pack[:7]
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, y if relu else None, weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, bias = ctx.saved_tensors
        w_krsc, scale, _, stride, pad, relu, owner = ctx.pack
        dy = dy.contiguous()
        need_x, need_res, need_w, need_b = ctx.needs_input_grad[:4]
        if relu or scale is not None or (ctx.has_res and need_res):
            d_conv, d_res = ops.act_bwd(dy, y, scale, relu=relu, want_res=ctx.has_res and need_res)
        else:
            d_conv, d_res = dy, None
        dx, dw, db = _conv_grads(x, d_conv, weight, bias, w_krsc, stride, pad, owner, need_x, need_w, need_b, bf16=ctx.bf16)
        return dx, d_res, dw, db, None


def _conv_grads(x, d_conv, weight, bias, w_krsc, stride, pad, owner, need_x, need_w, need_b, bf16=False):
    """(dx, dw, db) of one convolution from the gradient of its raw output: the filter and bias gradients where the installed
    schedule puts them (``_wgrad``), then the data gradient.  None for what is not needed."""
    dx = dw = db = None
    r, s = w_krsc.shape[1], w_krsc.shape[2]
    need_b = need_b and bias is not None
    if need_w or need_b:
        grads = _wgrad(x, d_conv, r, s, stride, pad, weight if need_w else None, bias if need_b else None, bf16=bf16)
        if need_w:
            dw = grads[0]
        if need_b:
            db = grads[-1]
    if need_x and bf16:
        dx = _bwd_data_bf16(d_conv, owner, w_krsc, tuple(x.shape), stride=stride, pad=pad)
    elif need_x:
        w_t = _transposed_filter(owner, w_krsc)
        dx = ops.conv2d_bwd_data(d_conv, w_t, tuple(x.shape), stride=stride, pad=pad,
                                 w_winograd=_dgrad_winograd(owner, w_t, tuple(x.shape), stride, pad))
    return dx, dw, db


class _BnTrainFn(torch.autograd.Function):
    """act(batch_norm(y, batch statistics) [+ residual]) - frcnn_bn_train_fwd / _bwd.  The module's running statistics
    are updated in place by the forward launch (F.batch_norm(training=True))."""

    @staticmethod
    def forward(ctx, y, residual, gamma, beta, bn, relu):
        track = bn.track_running_stats and bn.running_mean is not None
        momentum = bn.momentum
        sink = SCHEDULE.bn_stat_sink.get(id(bn)) if (track and SCHEDULE.bn_stat_sink is not None) else None
        if sink is not None:
            # deferred statistics (model/train_graph.TrainPipeline): this launch leaves the frame's batch mean / unbiased
            # variance in the slot's private buffers - momentum 1 turns the kernel's update (1 - m) * old + m * stat into
            # 0 * old + stat - and the running statistics are folded afterwards, in frame order
            run_mean, run_var, momentum = sink[0], sink[1], 1.0
            sink[2] = True          # this module really runs in the captured step (layer4's BatchNorms of the LiDAR net do not)
        else:
            run_mean, run_var = (bn.running_mean, bn.running_var) if track else (None, None)
            if track and bn.num_batches_tracked is not None:
                bn.num_batches_tracked += 1
                if momentum is None:                       # cumulative moving average (torch.nn.modules.batchnorm)
                    momentum = 1.0 / float(bn.num_batches_tracked)
        out, mean, invstd = ops.bn_train_fwd(y, gamma.detach() if gamma is not None else None,
                                             beta.detach() if beta is not None else None, bn.eps, momentum or 0.0,
                                             run_mean, run_var, residual, relu)
        if track and sink is None:
            bn.__dict__['_frcnn_stats_version'] = bn.__dict__.get('_frcnn_stats_version', 0) + 1
        ctx.relu = relu
        ctx.has_res = residual is not None
        ctx.affine = (gamma, beta)
        ctx.save_for_backward(y, out if relu else None, gamma, mean, invstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, out, gamma, mean, invstd = ctx.saved_tensors
        wprm, bprm = ctx.affine
        if (SCHEDULE.accumulate and BN_GRADS_IN_KERNEL and ctx.needs_input_grad[2] and ctx.needs_input_grad[3] and wprm is not None and bprm is not None
                and wprm.grad is not None and bprm.grad is not None and wprm.grad.is_contiguous() and bprm.grad.is_contiguous()):
            # captured steps: d_gamma / d_beta are added into the parameters' gradient buffers by the BatchNorm backward's own
            # statistics pass (no temporaries, no add_ launches: 168 of the LiDAR step's launches)
            dy, dres, _, _ = ops.bn_train_bwd(dout.contiguous(), out, y, gamma.detach() if gamma is not None else None, mean, invstd,
                                              relu=ctx.relu, want_res=ctx.has_res and ctx.needs_input_grad[1],
                                              grad_gamma=wprm.grad.view(-1), grad_beta=bprm.grad.view(-1))
            return dy if ctx.needs_input_grad[0] else None, dres, None, None, None, None
        dy, dres, dgamma, dbeta = ops.bn_train_bwd(dout.contiguous(), out, y, gamma.detach() if gamma is not None else None,
                                                   mean, invstd, relu=ctx.relu,
                                                   want_res=ctx.has_res and ctx.needs_input_grad[1])
        if SCHEDULE.accumulate:
            # captured steps (model/train_graph.py) accumulate parameter gradients themselves, in place, on the step's stream:
            # autograd's AccumulateGrad nodes run on the parameters' creation stream, outside the capture
            with torch.no_grad():
                for prm, g, need in ((ctx.affine[0], dgamma, ctx.needs_input_grad[2]), (ctx.affine[1], dbeta, ctx.needs_input_grad[3])):
                    if need and prm is not None and g is not None:
                        _accumulate(prm, g.view_as(prm))
            dgamma = dbeta = None
        return (dy if ctx.needs_input_grad[0] else None, dres, dgamma if ctx.needs_input_grad[2] else None,
                dbeta if ctx.needs_input_grad[3] else None, None, None)


def conv_bn_act_train(x, conv, bn=None, relu=False, residual=None, use_bn=True):
    """Differentiable counterpart of hip_modules.conv_bn_act.  An eval-mode (frozen) BatchNorm is folded into the
    convolution's epilogue; a BatchNorm in train() mode (LiDAR backbone, lib/nets/lidarnet.py:152-175) runs as its own
    node on the raw convolution output with batch statistics."""
    stride, pad = _stride_pad(conv)
    if bn is not None and use_bn and bn.training:
        w_krsc, _, shift = prepared_conv(conv, None, False)
        if x.shape[-1] != w_krsc.shape[-1]:
            raise NotImplementedError("differentiable conv needs C % 4 == 0 inputs (only the frozen stem pads its input)")
        y = _ConvFn.apply(x, None, conv.weight, conv.bias, (w_krsc, None, shift, stride, pad, False, conv, True))
        return _BnTrainFn.apply(y, residual, bn.weight, bn.bias, bn, relu)
    if bn is not None and use_bn and any(p.requires_grad for p in bn.parameters()):
        raise NotImplementedError("trainable BatchNorm affine parameters with frozen (eval-mode) statistics are not on "
                                  "the HIP path: the reference either freezes both or trains both")
    w_krsc, scale, shift = prepared_conv(conv, bn, use_bn)
    if x.shape[-1] != w_krsc.shape[-1]:
        raise NotImplementedError("differentiable conv needs C % 4 == 0 inputs (only the frozen stem pads its input)")
    # with a folded BN the effective bias is shift = bn.bias - mean*scale (+ conv.bias*scale); conv.bias itself only
    # exists on the BN-free convolutions (RPN, FPN), where shift == conv.bias and d(bias) = sum(d_conv)
    return _ConvFn.apply(x, residual, conv.weight, conv.bias, (w_krsc, scale, shift, stride, pad, relu, conv, True))


def linear_train(x2d, lin, relu=False, weight_nhwc_from=None):
    """act(x W^T + b) as a 1x1 convolution over R "pixels".  ``weight_nhwc_from=(C,P)`` says the Linear consumes an
    NCHW-flattened (C,P,P) map while ``x2d`` is the NHWC flattening: the filter columns are permuted once (cached)."""
    r, cin = x2d.shape
    if weight_nhwc_from is None:
        w_krsc = lin.weight.detach().view(lin.out_features, 1, 1, cin)
        return _ConvFn.apply(x2d.view(r, 1, 1, cin), None, lin.weight, lin.bias,
                             (w_krsc, None, lin.bias.detach(), 1, 0, relu, lin)).view(r, -1)
    return _PermutedLinearFn.apply(x2d, lin.weight, lin.bias, lin, weight_nhwc_from, relu)


class _PermutedLinearFn(torch.autograd.Function):
    @staticmethod
    def _prepared(lin, c, p):
        key = (lin.weight._version, lin.weight.data_ptr())
        cache = lin.__dict__.get('_frcnn_perm')
        if cache is not None and cache[0] == key:
            return cache[1][0]
        w = lin.weight.detach().view(lin.out_features, c, p, p).permute(0, 2, 3, 1).reshape(lin.out_features, 1, 1, -1)
        return stable_store(lin, '_frcnn_perm', key, (w.contiguous(),),
                            refresh=lambda: _PermutedLinearFn._prepared(lin, c, p))[0]

    @staticmethod
    def forward(ctx, x2d, weight, bias, lin, cp, relu):
        c, p = cp
        w_krsc = _PermutedLinearFn._prepared(lin, c, p)
        r = x2d.shape[0]
        y = ops.conv2d_nhwc(x2d.view(r, 1, 1, -1), w_krsc, None, bias.detach(), None, relu=relu)
        ctx.meta = (lin, cp, relu, w_krsc)
        ctx.save_for_backward(x2d, y if relu else None)
        return y.view(r, -1)

    @staticmethod
    def backward(ctx, dy):
        x2d, y = ctx.saved_tensors
        lin, (c, p), relu, w_krsc = ctx.meta
        r = x2d.shape[0]
        dy4 = dy.contiguous().view(r, 1, 1, -1)
        d_conv = ops.act_bwd(dy4, y, None, relu=True)[0] if relu else dy4
        x4 = x2d.view(r, 1, 1, -1)
        to_w = lambda dwk, dbk: dwk.view(lin.out_features, p, p, c).permute(0, 3, 1, 2).reshape(lin.out_features, -1)
        dw, db = _wgrad(x4, d_conv, 1, 1, 1, 0, mapped=[(lin.weight, to_w), (lin.bias, lambda dwk, dbk: dbk)])
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.conv2d_bwd_data(d_conv, _transposed_filter(lin, w_krsc), tuple(x4.shape)).view(r, -1)
        return dx, dw, db, None, None, None


class _FusedHeadFn(torch.autograd.Function):
    """Two sibling layers that share their input (rpn_cls_score_net + rpn_bbox_pred_net, cls_score_net +
    bbox_pred_net) as ONE convolution with the filters concatenated along K and zero-padded to a multiple of 4."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, pack):
        w_krsc, bias_cat, owner = pack
        y = ops.conv2d_nhwc(x, w_krsc, None, bias_cat, None)
        ctx.pack = pack
        ctx.biases = (b1, b2)
        ctx.save_for_backward(x, w1, w2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2 = ctx.saved_tensors
        w_krsc, _, owner = ctx.pack
        dy = dy.contiguous()
        k1, k2 = w1.shape[0], w2.shape[0]
        b1, b2 = ctx.biases
        dw1, db1, dw2, db2 = _wgrad(x, dy, w_krsc.shape[1], w_krsc.shape[2], 1, 0, mapped=[
            (w1, lambda dwk, dbk: _param_grad_from_krsc(dwk[:k1], w1)),
            (b1, lambda dwk, dbk: dbk[:k1].contiguous()),
            (w2, lambda dwk, dbk: _param_grad_from_krsc(dwk[k1:k1 + k2], w2)),
            (b2, lambda dwk, dbk: dbk[k1:k1 + k2].contiguous())])
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.conv2d_bwd_data(dy, _transposed_filter(owner, w_krsc), tuple(x.shape))
        return dx, dw1, db1, dw2, db2, None


def fused_head_weights(owner, m1, m2, cache_name):
    """(w_krsc (K1+K2 padded to %4, 1, 1, C), bias) of two 1x1-conv / Linear siblings, cached on ``owner``."""
    tensors = (m1.weight, m1.bias, m2.weight, m2.bias)
    key = tuple((t._version, t.data_ptr()) for t in tensors)
    cache = owner.__dict__.get(cache_name)
    if cache is not None and cache[0] == key:
        return cache[1]
    with torch.no_grad():
        w1 = m1.weight.detach().reshape(m1.weight.shape[0], -1)
        w2 = m2.weight.detach().reshape(m2.weight.shape[0], -1)
        k = w1.shape[0] + w2.shape[0]
        kp = pad4(k)
        w = torch.zeros((kp, w1.shape[1]), dtype=torch.float32, device=w1.device)
        w[:w1.shape[0]] = w1
        w[w1.shape[0]:k] = w2
        b = torch.zeros((kp,), dtype=torch.float32, device=w1.device)
        b[:w1.shape[0]] = m1.bias.detach()
        b[w1.shape[0]:k] = m2.bias.detach()
        w = w.view(kp, 1, 1, -1).contiguous()
    return stable_store(owner, cache_name, key, (w, b), refresh=lambda: fused_head_weights(owner, m1, m2, cache_name))


def fused_head_train(x, owner, m1, m2, cache_name):
    w, b = fused_head_weights(owner, m1, m2, cache_name)
    return _FusedHeadFn.apply(x, m1.weight, m1.bias, m2.weight, m2.bias, (w, b, _Holder.of(owner, cache_name)))


class _Holder(object):
    """Small attribute bag that owns the transposed-filter cache of a fused head."""
    @staticmethod
    def of(owner, name):
        h = owner.__dict__.get(name + '_holder')
        if h is None:
            h = _Holder()
            owner.__dict__[name + '_holder'] = h
        return h


class _BottleneckFn(torch.autograd.Function):
    """lib/nets/resnet.py:98-127 as one node: three (four with the projection shortcut) fused conv launches forward;
    backward walks them in reverse and accumulates the two gradients of the block input inside the last
    data-gradient launch."""

    @staticmethod
    def forward(ctx, x, block, use_bn, *weights):
        p1 = prepared_conv(block.conv1, block.bn1, use_bn)
        p2 = prepared_conv(block.conv2, block.bn2, use_bn)
        p3 = prepared_conv(block.conv3, block.bn3, use_bn)
        s1, _ = _stride_pad(block.conv1)
        s2, _ = _stride_pad(block.conv2)
        # cfg.TRAIN.CONV_BF16, per convolution (conv1, conv2, conv3, projection): a trainable filter, or a gradient passes through
        need = ctx.needs_input_grad
        g1 = need[0] or need[3]
        g2 = g1 or need[4]
        g3 = g2 or need[5]
        if block.downsample is not None:
            pd = prepared_conv(block.downsample[0], block.downsample[1], True)
            sd, _ = _stride_pad(block.downsample[0])
            bfd = conv_bf16_train_wanted(pd[0], sd, 0, need[0] or need[6])
            if bfd:
                identity = _conv_fwd_bf16(x, pd, block.downsample[0], None, sd, 0, False)
            else:
                identity = ops.conv2d_nhwc(x, pd[0], pd[1], pd[2], None, stride=sd, pad=0, relu=False)
        else:
            pd, sd, identity, bfd = None, 1, x, False
        bf = (conv_bf16_train_wanted(p1[0], s1, 0, g1), conv_bf16_train_wanted(p2[0], s2, 1, g2),
              conv_bf16_train_wanted(p3[0], 1, 0, g3), bfd)
        if bf[0]:
            o1 = _conv_fwd_bf16(x, p1, block.conv1, None, s1, 0, True)
        else:
            o1 = ops.conv2d_nhwc(x, p1[0], p1[1], p1[2], None, stride=s1, pad=0, relu=True)
        if bf[1]:
            o2 = _conv_fwd_bf16(o1, p2, block.conv2, None, s2, 1, True)
        else:
            # the 3x3 layer with its cached Winograd-transformed filter when its tuned plan reads one (re-derived only when the
            # weights change, i.e. once per optimizer step instead of inside every call)
            u2 = _winograd_filter(block.conv2, p2[0], tuple(o1.shape[:3]), s2, 1)
            o2 = ops.conv2d_nhwc(o1, p2[0], p2[1], p2[2], None, stride=s2, pad=1, relu=True, w_winograd=u2)
        if bf[2]:
            out = _conv_fwd_bf16(o2, p3, block.conv3, identity, 1, 0, True)
        else:
            out = ops.conv2d_nhwc(o2, p3[0], p3[1], p3[2], identity, stride=1, pad=0, relu=True)
        ctx.bf16 = bf
        ctx.block = block
        ctx.meta = (p1, p2, p3, pd, s1, s2, sd)
        ctx.save_for_backward(x, o1, o2, out)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, o1, o2, out = ctx.saved_tensors
        blk = ctx.block
        p1, p2, p3, pd, s1, s2, sd = ctx.meta
        need_w = [w.requires_grad for w in (blk.conv1.weight, blk.conv2.weight, blk.conv3.weight)]

        bf = ctx.bf16     # (conv1, conv2, conv3, projection) run with bf16 operands: the forward's answer holds for the gradients

        def wg(inp, dz, conv, r, stride, pad, bf16=False):
            return _wgrad(inp, dz, r, r, stride, pad, conv.weight, bf16=bf16)[0]

        dz3, d_id = ops.act_bwd(dy.contiguous(), out, p3[1], relu=True, want_res=True)
        dw3 = wg(o2, dz3, blk.conv3, 1, 1, 0, bf[2]) if need_w[2] else None
        # the ReLU / folded-BatchNorm backward of conv2 (conv1) is applied by the data-gradient launch of conv3 (conv2) as it
        # stores its result (frcnn_conv2d_bwd_data_act): no separate pass over d_o2 / d_o1
        if bf[2]:
            dz2 = _bwd_data_bf16(dz3, blk.conv3, p3[0], tuple(o2.shape), act_y=o2, act_scale=p2[1])
        else:
            w3_t = _transposed_filter(blk.conv3, p3[0])
            if FUSE_ACT_BWD:
                dz2 = ops.conv2d_bwd_data(dz3, w3_t, tuple(o2.shape), act_y=o2, act_scale=p2[1])
            else:
                dz2, _ = ops.act_bwd(ops.conv2d_bwd_data(dz3, w3_t, tuple(o2.shape)), o2, p2[1], relu=True)
        dw2 = wg(o1, dz2, blk.conv2, 3, s2, 1, bf[1]) if need_w[1] else None
        if bf[1]:
            dz1 = _bwd_data_bf16(dz2, blk.conv2, p2[0], tuple(o1.shape), stride=s2, pad=1, act_y=o1, act_scale=p1[1])
        else:
            w2_t = _transposed_filter(blk.conv2, p2[0])
            u2_t = _dgrad_winograd(blk.conv2, w2_t, tuple(o1.shape), s2, 1)
            if FUSE_ACT_BWD:
                dz1 = ops.conv2d_bwd_data(dz2, w2_t, tuple(o1.shape), stride=s2, pad=1, w_winograd=u2_t, act_y=o1, act_scale=p1[1])
            else:
                dz1, _ = ops.act_bwd(ops.conv2d_bwd_data(dz2, w2_t, tuple(o1.shape), stride=s2, pad=1, w_winograd=u2_t), o1, p1[1],
                                     relu=True)
        dw1 = wg(x, dz1, blk.conv1, 1, s1, 0, bf[0]) if need_w[0] else None
        dwd = None
        dx = None

        def dgrad(dz, conv, prepared, stride, add, bf16):
            if bf16:
                return _bwd_data_bf16(dz, conv, prepared[0], tuple(x.shape), stride=stride, add=add)
            return ops.conv2d_bwd_data(dz, _transposed_filter(conv, prepared[0]), tuple(x.shape), stride=stride, add=add)

        if pd is not None:
            dzd, _ = ops.act_bwd(d_id, None, pd[1], relu=False)
            if blk.downsample[0].weight.requires_grad:
                dwd = wg(x, dzd, blk.downsample[0], 1, sd, 0, bf[3])
            if ctx.needs_input_grad[0]:
                dx = dgrad(dzd, blk.downsample[0], pd, sd, None, bf[3])
                dx = dgrad(dz1, blk.conv1, p1, s1, dx, bf[0])
        elif ctx.needs_input_grad[0]:
            dx = dgrad(dz1, blk.conv1, p1, s1, d_id, bf[0])
        grads = [dw1, dw2, dw3]     # parameter-layout gradients, or None when they were accumulated on the side stream
        if pd is not None:
            grads.append(dwd)
        return (dx, None, None) + tuple(grads)


def bottleneck_train(x, block):
    """Differentiable Bottleneck.  With every BatchNorm frozen (image detector) or absent (LiDAR layer4) the block is
    ONE autograd node; a block holding a BatchNorm in train() mode is the chain conv -> batch-norm node per layer."""
    bn_on = block.batchnorm_en
    live = [bn for bn in (block.bn1, block.bn2, block.bn3) if bn_on and bn.training]
    if block.downsample is not None and block.downsample[1].training:
        live.append(block.downsample[1])
    if live:
        if block.downsample is not None:
            identity = conv_bn_act_train(x, block.downsample[0], block.downsample[1], relu=False)
        else:
            identity = x
        out = conv_bn_act_train(x, block.conv1, block.bn1, relu=True, use_bn=bn_on)
        out = conv_bn_act_train(out, block.conv2, block.bn2, relu=True, use_bn=bn_on)
        return conv_bn_act_train(out, block.conv3, block.bn3, relu=True, residual=identity, use_bn=bn_on)
    weights = [block.conv1.weight, block.conv2.weight, block.conv3.weight]
    if block.downsample is not None:
        weights.append(block.downsample[0].weight)
    return _BottleneckFn.apply(x, block, block.batchnorm_en, *weights)


class _SeparablePairFn(torch.autograd.Function):
    """One depthwise-separable child of MobileNet-v1 (lib/nets/mobilenet_v1.py:117-132) as one node, BatchNorms frozen and
    folded: a = relu6(bn(dw(min(x, in_cap)))), b = relu(bn(pw(a))) with b's upper clamp PENDING - the next child reads
    min(b, 6) through its ``in_cap`` - unless ``finish_cap``: then the node applies it in place (Conv2d_11, read by the RPN
    and the RoIAlign; Conv2d_13, read by the spatial mean).  Either way the incoming gradient is the one with respect to
    min(b, 6), and 0 < b < 6 is the ReLU6 mask whether or not b has been clamped."""

    @staticmethod
    def forward(ctx, x, pair, in_cap, finish_cap, dw_weight, pw_weight):
        dw, pw = pair.depthwise[0], pair.pointwise[0]
        wd, sd, bd = prepared_depthwise(dw, pair.depthwise[1])
        wp, sp, bp = prepared_conv(pw, pair.pointwise[1], True)
        stride = dw.stride[0]
        a = ops.depthwise_conv3x3_nhwc(x, wd, sd, bd, stride=stride, relu=True, in_cap=in_cap, out_cap=RELU6_CAP)
        b = ops.conv2d_nhwc(a, wp, sp, bp, None, stride=1, pad=0, relu=True)
        if finish_cap:
            ops.clamp_max_(b, RELU6_CAP)
        ctx.pair = pair
        ctx.meta = (wd, sd, wp, sp, stride, in_cap)
        ctx.save_for_backward(x, a, b)
        return b

    @staticmethod
    def backward(ctx, db):
        x, a, b = ctx.saved_tensors
        dw, pw = ctx.pair.depthwise[0], ctx.pair.pointwise[0]
        wd, sd, wp, sp, stride, in_cap = ctx.meta
        need_x, need_dw, need_pw = ctx.needs_input_grad[0], ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        d_pw = ops.act_bwd_cap(db.contiguous(), b, sp, relu=True, cap=RELU6_CAP)
        g_pw = _wgrad(a, d_pw, 1, 1, 1, 0, pw.weight)[0] if need_pw else None
        dx = g_dw = None
        if need_x or need_dw:
            da = ops.conv2d_bwd_data(d_pw, _transposed_filter(pw, wp), tuple(a.shape))
            if need_dw:
                def filter_grad(out=None, accumulate=False):
                    return ops.depthwise_conv3x3_bwd_weight(x, da, a, sd, stride=stride, relu=True, in_cap=in_cap,
                                                            out_cap=RELU6_CAP, out=out, accumulate=accumulate)
                grad = dw.weight.grad
                if not SCHEDULE.accumulate:
                    g_dw = filter_grad()
                elif grad is not None and grad.is_contiguous():
                    # the kernel's own second launch adds into param.grad: no permute, no add_ launch
                    _launch_wgrad(grad, [x, da, a], lambda: filter_grad(grad, True))
                else:
                    _launch_wgrad(dw.weight, [x, da, a], lambda: _accumulate(dw.weight, filter_grad()))
            if need_x:
                dx = ops.depthwise_conv3x3_bwd_data(da, a, wd, tuple(x.shape), sd, stride=stride, relu=True, out_cap=RELU6_CAP)
        return dx, None, None, None, g_dw, g_pw


def separable_pair_train(x, pair, in_cap, finish_cap):
    """Differentiable depthwise-separable child; ``x`` NHWC with the upper clamp ``in_cap`` pending (inf: none)."""
    for bn in (pair.depthwise[1], pair.pointwise[1]):
        if bn.training:
            raise NotImplementedError("BatchNorm in training mode (batch statistics) is not on the HIP path yet")
        if any(p.requires_grad for p in bn.parameters()):
            raise NotImplementedError("trainable BatchNorm affine parameters with frozen (eval-mode) statistics are not on "
                                      "the HIP path: the reference either freezes both or trains both")
    return _SeparablePairFn.apply(x, pair, float(in_cap), bool(finish_cap), pair.depthwise[0].weight, pair.pointwise[0].weight)


class _MaxPoolFn(torch.autograd.Function):
    """nn.MaxPool2d(3, 2, 1) of the stem (lib/nets/resnet.py:156) when the stem trains (FIXED_BLOCKS == -1)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.maxpool3x3s2_nhwc(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.maxpool3x3s2_bwd(x, dy.contiguous())


def maxpool_train(x):
    return _MaxPoolFn.apply(x)


class _MaxPool2x2Fn(torch.autograd.Function):
    """nn.MaxPool2d(2, 2) of the VGG16 body (lib/nets/vgg16.py:35,46) behind something other than a trained convolution."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.maxpool2x2s2_nhwc(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.maxpool2x2s2_bwd(x, dy.contiguous())


def maxpool2x2_train(x):
    return _MaxPool2x2Fn.apply(x)


class _ConvReluPoolFn(torch.autograd.Function):
    """p = maxpool2x2(relu(conv(x, w) + b)) as one node (VGG16's features.14 + pool 16, features.21 + pool 23).  y, the ReLU
    output, is both the pool's input and the ReLU's mask, so the pool's backward writes the gradient of the convolution's raw
    output directly (``maxpool2x2s2_bwd(relu=True)``): the full-size gradient of y is never written and re-read by an
    ``act_bwd`` pass."""

    @staticmethod
    def forward(ctx, x, weight, bias, pack):
        w_krsc, shift, stride, pad, owner = pack
        u = _winograd_filter(owner, w_krsc, tuple(x.shape[:3]), stride, pad) if w_krsc.shape[1] == 3 else None
        y = ops.conv2d_nhwc(x, w_krsc, None, shift, None, stride=stride, pad=pad, relu=True, w_winograd=u)
        ctx.pack = pack
        ctx.save_for_backward(x, y, weight, bias)
        return ops.maxpool2x2s2_nhwc(y)

    @staticmethod
    def backward(ctx, dp):
        x, y, weight, bias = ctx.saved_tensors
        w_krsc, _, stride, pad, owner = ctx.pack
        d_conv = ops.maxpool2x2s2_bwd(y, dp.contiguous(), relu=True)
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx, dw, db = _conv_grads(x, d_conv, weight, bias, w_krsc, stride, pad, owner, need_x, need_w, need_b)
        return dx, dw, db, None


def conv_relu_pool_train(x, conv):
    """Differentiable ``MaxPool2d(2, 2)(relu(conv(x)))`` of a convolution with a bias and no BatchNorm."""
    stride, pad = _stride_pad(conv)
    w_krsc, scale, shift = prepared_conv(conv, None, False)
    if scale is not None or x.shape[-1] != w_krsc.shape[-1]:
        raise NotImplementedError("conv_relu_pool_train: a convolution without BatchNorm on a C % 4 == 0 input")
    return _ConvReluPoolFn.apply(x, conv.weight, conv.bias, (w_krsc, shift, stride, pad, conv))


class _DropoutFn(torch.autograd.Function):
    """nn.Dropout(p) in train() mode with counter-based masks (frcnn_dropout_fwd / _bwd): the draws use ``seed + *seed_dev``
    (Network.uc_seed_args), so a captured step draws a new mask per replay."""

    @staticmethod
    def forward(ctx, x, p, seed, stream, seed_dev=None):
        ctx.meta = (p, seed, stream, seed_dev)
        return ops.dropout(x.contiguous(), p, seed, stream, seed_dev=seed_dev)

    @staticmethod
    def backward(ctx, dy):
        p, seed, stream, seed_dev = ctx.meta
        return ops.dropout_bwd(dy.contiguous(), p, seed, stream, seed_dev=seed_dev), None, None, None, None


class _UpsampleAddFn(torch.autograd.Function):
    """lib/nets/fpn.py:42-45."""

    @staticmethod
    def forward(ctx, x, lateral):
        ctx.in_hw = (x.shape[1], x.shape[2])
        return ops.upsample_bilinear_add(x, lateral)

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        dx = ops.upsample_bilinear_bwd(dout, ctx.in_hw) if ctx.needs_input_grad[0] else None
        return dx, (dout if ctx.needs_input_grad[1] else None)


def upsample_add_train(x, lateral):
    return _UpsampleAddFn.apply(x, lateral)


class _MultiLevelRoIAlignFn(torch.autograd.Function):
    """MultiScaleRoIAlign.forward (lib/utils/torchpoolers.py:137-200): every level writes the RoIs mapped to it."""

    @staticmethod
    def forward(ctx, rois, levels, meta, *feats):
        pooled, scales, sampling = meta
        out = torch.zeros((rois.shape[0], pooled, pooled, feats[0].shape[-1]), dtype=torch.float32, device=rois.device)
        for lvl, (f, sc) in enumerate(zip(feats, scales)):
            ops.roi_align_nhwc(f, rois, pooled, sc, sampling, level_of_roi=levels, level=lvl if levels is not None else -1,
                               out=out)
        ctx.meta = meta
        ctx.shapes = [tuple(f.shape) for f in feats]
        ctx.save_for_backward(rois, levels)
        return out

    @staticmethod
    def backward(ctx, dout):
        rois, levels = ctx.saved_tensors
        pooled, scales, sampling = ctx.meta
        dout = dout.contiguous()
        grads = []
        for lvl, (shape, sc) in enumerate(zip(ctx.shapes, scales)):
            if not ctx.needs_input_grad[3 + lvl]:
                grads.append(None)
                continue
            grads.append(ops.roi_align_bwd(dout, shape, rois, sc, sampling, level_of_roi=levels,
                                           level=lvl if levels is not None else -1))
        return (None, None, None) + tuple(grads)


def roi_align_train(feats, rois, levels, pooled, scales, sampling):
    return _MultiLevelRoIAlignFn.apply(rois, levels, (pooled, tuple(scales), sampling), *feats)


class _SpatialMeanFn(torch.autograd.Function):
    """fc7 = layer4(pool5).mean(3).mean(2) (tail of the non-FPN detector)."""

    @staticmethod
    def forward(ctx, x):
        ctx.pooled = x.shape[1]
        return ops.spatial_mean(x)

    @staticmethod
    def backward(ctx, dout):
        return ops.spatial_mean_bwd(dout.contiguous(), ctx.pooled)


def spatial_mean_train(x):
    return _SpatialMeanFn.apply(x)


class _GatherPatchesFn(torch.autograd.Function):
    """The r x s windows of a (1,H,W,C) map around a device-side list of pixels (ops.gather_patches); backward scatters the
    window gradients back into a zero map (float atomics, like the RoIAlign backward)."""

    @staticmethod
    def forward(ctx, x, idx, count, r, s, pad):
        ctx.meta = (x.shape[1], x.shape[2], pad)
        ctx.save_for_backward(idx, count)
        return ops.gather_patches(x, idx, count, r, s, pad)

    @staticmethod
    def backward(ctx, d):
        idx, count = ctx.saved_tensors
        h, w, pad = ctx.meta
        return ops.scatter_add_patches(d.contiguous(), idx, count, h, w, pad), None, None, None, None, None


def conv_on_patches_train(x, idx, count, conv, holder, relu=True):
    """act(conv(x)) at the listed pixels ONLY, differentiable: a stride-1 padded convolution evaluated at pixel p is the VALID
    convolution of the r x s window around p, so the result (cap, 1, 1, K) equals rows ``idx`` of the dense output and its
    backward costs cap output pixels instead of H x W.  ``holder`` owns the caches of this form (the dense form of the same
    module keeps its own on the module)."""
    r, s = conv.kernel_size
    stride, pad = _stride_pad(conv)
    if stride != 1:
        raise NotImplementedError("conv_on_patches_train: stride-1 convolutions only")
    patches = _GatherPatchesFn.apply(x, idx, count, r, s, pad)
    w_krsc, _, shift = prepared_conv(conv, None, False)
    return _ConvFn.apply(patches, None, conv.weight, conv.bias, (w_krsc, None, shift, 1, 0, relu, holder))


class _RpnLossFn(torch.autograd.Function):
    """cross_entropy over labelled anchors + smooth_l1_loss('RPN', ...) on the fused RPN head output."""

    @staticmethod
    def forward(ctx, rpn2d, labels, targets, inside, outside, num_anchors):
        losses, drpn = ops.rpn_loss(rpn2d, num_anchors, labels, targets, inside, outside, 1.0, 1.0, want_grad=True)
        ctx.a = num_anchors
        ctx.save_for_backward(drpn)
        return losses[:2].clone()

    @staticmethod
    def backward(ctx, g):
        (drpn,) = ctx.saved_tensors
        a = ctx.a
        d = drpn.clone()
        d[:, :2 * a] *= g[0]          # cross-entropy gradient lives in the logit columns,
        d[:, 2 * a:6 * a] *= g[1]     # the box-loss gradient in the delta columns
        return d, None, None, None, None, None


def rpn_loss_train(rpn2d, labels, targets, inside, outside, num_anchors):
    return _RpnLossFn.apply(rpn2d, labels, targets, inside, outside, num_anchors)


class _DetLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cls_score, bbox_pred, labels, targets, inside, outside, lidar):
        losses, dcls, dbox = ops.det_loss(cls_score, labels, bbox_pred, targets, inside, outside, 4, 1.0, 1.0, lidar=lidar)
        ctx.save_for_backward(dcls, dbox)
        return losses

    @staticmethod
    def backward(ctx, g):
        dcls, dbox = ctx.saved_tensors
        return dcls * g[0], dbox * g[1], None, None, None, None, None


def det_loss_train(cls_score, bbox_pred, labels, targets, inside, outside, lidar=None):
    """``lidar=(REG_LOSS_WEIGHT, EN_RY_SIN)`` selects the 7-element form of lib/utils/loss_utils.py:61-77."""
    return _DetLossFn.apply(cls_score.contiguous(), bbox_pred.contiguous(), labels, targets, inside, outside, lidar)
