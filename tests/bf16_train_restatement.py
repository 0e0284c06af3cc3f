"""What cfg.TRAIN.CONV_BF16 computes, restated on the host: a convolution whose forward and whose two gradients multiply
bf16-rounded operands, in whatever dtype the caller's tensors have (float64 for the reference, float32 for the yardstick).

    y  = conv2d(r(x), r(w))
    dx = conv_transpose2d(r(dy), r(w))        (unrounded operands where ``round_dgrad`` is False: the strided 1x1 data gradient
                                               stays fp32 on the device)
    dw = sum over pixels of r(dy) * r(patch(x))

r(t) = t.to(torch.bfloat16) (round to nearest even) back in t's dtype.  The definition is straight-through: each gradient is the
gradient of the rounded product, the rounding itself has derivative one.

``small_net`` is the net of tests/test_train_conv_bf16.py on NCHW host tensors: a 3x3 convolution with C = 8 (not eligible:
plain products), a 1x1 convolution 64 -> 64 with a bias, then two Bottlenecks (lib/nets/resnet.py:98-127 with frozen
BatchNorms folded into scale / shift), the first with a stride-2 3x3 and a stride-2 1x1 projection.

CPU test (tests/test_bf16_train_restatement.py): on operands bf16 represents exactly the function and its gradients equal
plain float64 conv2d autograd exactly.
"""
import torch
import torch.nn.functional as F


def rbf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class Bf16Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, pad, round_dgrad):
        ctx.save_for_backward(x, w)
        ctx.meta = (stride, pad, round_dgrad)
        return F.conv2d(rbf16(x), rbf16(w), None, stride, pad)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad, round_dgrad = ctx.meta
        dx = dw = None
        if ctx.needs_input_grad[0]:
            if round_dgrad:
                dx = torch.nn.grad.conv2d_input(x.shape, rbf16(w), rbf16(dy), stride, pad)
            else:
                dx = torch.nn.grad.conv2d_input(x.shape, w, dy, stride, pad)
        if ctx.needs_input_grad[1]:
            dw = torch.nn.grad.conv2d_weight(rbf16(x), w.shape, rbf16(dy), stride, pad)
        return dx, dw, None, None, None


def conv_bf16(x, w, stride=1, pad=0, round_dgrad=True):
    return Bf16Conv.apply(x, w, stride, pad, round_dgrad)


def eligible(w):
    """nets/hip_modules.conv_bf16_train_eligible for a (K,C,R,S) filter with a gradient."""
    return w.shape[0] % 32 == 0 and w.shape[1] % 32 == 0


def conv(x, w, stride, pad, bf16):
    """One convolution of the net: bf16 products when the switch is on and the layer eligible, plain products otherwise; the
    strided 1x1 data gradient is plain either way."""
    if bf16 and eligible(w):
        return conv_bf16(x, w, stride, pad, round_dgrad=not (stride > 1 and w.shape[2] == 1 and w.shape[3] == 1))
    return F.conv2d(x, w, None, stride, pad)


def affine(y, scale, shift):
    if scale is not None:
        y = y * scale.view(1, -1, 1, 1)
    return y + shift.view(1, -1, 1, 1) if shift is not None else y


def bottleneck(x, p, prefix, stride, bf16, pre=None):
    """``p``: name -> tensor in x's dtype: '<prefix>.conv{1,2,3}.weight', '<prefix>.bn{1,2,3}.{scale,shift}' and, with a
    projection, '<prefix>.downsample.0.weight' / '<prefix>.downsample.1.{scale,shift}'.  ``pre``: list that receives the
    pre-activations."""
    pre = pre if pre is not None else []
    g = lambda name: p[prefix + '.' + name]
    if prefix + '.downsample.0.weight' in p:
        identity = affine(conv(x, g('downsample.0.weight'), stride, 0, bf16), g('downsample.1.scale'), g('downsample.1.shift'))
    else:
        identity = x
    t = affine(conv(x, g('conv1.weight'), 1, 0, bf16), g('bn1.scale'), g('bn1.shift'))
    pre.append(t)
    t = affine(conv(F.relu(t), g('conv2.weight'), stride, 1, bf16), g('bn2.scale'), g('bn2.shift'))
    pre.append(t)
    t = affine(conv(F.relu(t), g('conv3.weight'), 1, 0, bf16), g('bn3.scale'), g('bn3.shift')) + identity
    pre.append(t)
    return F.relu(t)


def small_net(x, p, bf16, pre=None, stages=None):
    """The test net.  ``stages``: list that receives the output of the ineligible front convolution."""
    pre = pre if pre is not None else []
    t = affine(conv(x, p['conv0.weight'], 1, 1, bf16), None, p['conv0.bias'])
    pre.append(t)
    t = F.relu(t)
    if stages is not None:
        stages.append(t)
    t = affine(conv(t, p['conv0b.weight'], 1, 0, bf16), None, p['conv0b.bias'])
    pre.append(t)
    t = bottleneck(F.relu(t), p, 'a', 2, bf16, pre)
    return bottleneck(t, p, 'b', 1, bf16, pre)
