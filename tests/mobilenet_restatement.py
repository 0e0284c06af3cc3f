"""MobileNet-v1 body restated on the CPU with torch functional calls, from the table of lib/nets/mobilenet_v1.py:33-49
(no module of the package or of the reference is used): Conv2d_0 = 3x3 / stride 2 / pad 1 convolution 3 -> 32, then 13
pairs of depthwise 3x3 (groups == C, pad 1) and pointwise 1x1, every convolution bias-free and followed by an eval-mode
BatchNorm (eps 1e-5) and ReLU6.  Runs in fp32 and float64.  Also the seeded weight procedure shared by
tests/golden/make_golden_mobilenet.py (which fills the reference's modules with it) and the tests.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

STEM = (2, 32)
PAIRS = ((1, 64), (2, 128), (1, 128), (2, 256), (1, 256), (2, 512), (1, 512), (1, 512), (1, 512), (1, 512), (1, 512),
         (1, 1024), (1, 1024))
HEAD_CHILDREN = 12
BN_EPS = 1e-5
SEED = 20261


def _bn_keys(prefix, c):
    return [(prefix + '.weight', (c,)), (prefix + '.bias', (c,)), (prefix + '.running_mean', (c,)),
            (prefix + '.running_var', (c,)), (prefix + '.num_batches_tracked', ())]


def key_shapes():
    """[(state-dict key, shape)] of the body in module order."""
    out = [('Conv2d_0.0.weight', (STEM[1], 3, 3, 3))] + _bn_keys('Conv2d_0.1', STEM[1])
    cin = STEM[1]
    for i, (_, depth) in enumerate(PAIRS, 1):
        out += [('Conv2d_%d.depthwise.0.weight' % i, (cin, 1, 3, 3))] + _bn_keys('Conv2d_%d.depthwise.1' % i, cin)
        out += [('Conv2d_%d.pointwise.0.weight' % i, (depth, cin, 1, 1))] + _bn_keys('Conv2d_%d.pointwise.1' % i, depth)
        cin = depth
    return out


def seeded_state(shapes=None, seed=SEED):
    """Weights from names and shapes alone: one numpy ``default_rng(seed)`` stream, tensors visited in SORTED key order.
    Convolution weights N(0, sqrt(2 / fan_in)), BatchNorm weights U(0.8, 1.6), biases N(0.2, 0.2), running means
    N(0, 0.1), running variances U(0.5, 1.5), num_batches_tracked 0.  Returns an OrderedDict (in the order of ``shapes``) of
    float64 numpy arrays (int64 for the counters)."""
    shapes = key_shapes() if shapes is None else [(k, tuple(int(v) for v in s)) for k, s in shapes]
    rng = np.random.default_rng(seed)
    made = {}
    for key, shape in sorted(shapes):
        if key.endswith('num_batches_tracked'):
            made[key] = np.zeros(shape, dtype=np.int64)
        elif len(shape) == 4:
            made[key] = rng.normal(0.0, np.sqrt(2.0 / (shape[1] * shape[2] * shape[3])), shape)
        elif key.endswith('.weight'):
            made[key] = rng.uniform(0.8, 1.6, shape)
        elif key.endswith('.bias'):
            made[key] = rng.normal(0.2, 0.2, shape)
        elif key.endswith('running_mean'):
            made[key] = rng.normal(0.0, 0.1, shape)
        elif key.endswith('running_var'):
            made[key] = rng.uniform(0.5, 1.5, shape)
        else:
            raise KeyError(key)
    return OrderedDict((k, made[k]) for k, _ in shapes)


def torch_state(state, dtype=torch.float32):
    return OrderedDict((k, torch.from_numpy(np.asarray(v)).to(dtype if v.dtype.kind == 'f' else torch.int64))
                       for k, v in state.items())


def checksums(state):
    """float64 sum of v * (1 + (i mod 7)) over the flattened tensor, per key: order-sensitive, cheap to store."""
    out = OrderedDict()
    for k, v in state.items():
        flat = np.asarray(v, dtype=np.float64).ravel()
        out[k] = float(np.sum(flat * (1.0 + np.arange(flat.size) % 7)))
    return out


def _conv_bn_relu6(x, state, prefix, stride, pad, groups):
    w = state[prefix + '.0.weight'].to(x.dtype)
    y = F.conv2d(x, w, None, stride, pad, 1, groups)
    g, b, m, v = (state[prefix + '.1.' + k].to(x.dtype).view(1, -1, 1, 1)
                  for k in ('weight', 'bias', 'running_mean', 'running_var'))
    y = (y - m) / torch.sqrt(v + BN_EPS) * g + b
    return y.clamp(0, 6)


def run(state, x, first=0, last=14, stages=None):
    """Children [first:last] of the body on the NCHW tensor ``x`` (its dtype is the evaluation's precision).  ``stages``:
    a list that receives every child's output."""
    for i in range(first, last):
        if i == 0:
            x = _conv_bn_relu6(x, state, 'Conv2d_0', STEM[0], 1, 1)
        else:
            x = _conv_bn_relu6(x, state, 'Conv2d_%d.depthwise' % i, PAIRS[i - 1][0], 1, x.shape[1])
            x = _conv_bn_relu6(x, state, 'Conv2d_%d.pointwise' % i, 1, 0, 1)
        if stages is not None:
            stages.append(x)
    return x


def head(state, x, stages=None):
    return run(state, x, 0, HEAD_CHILDREN, stages)


def tail(state, pooled, stages=None):
    """Children [12:] on the pooled RoIs, then .mean(3).mean(2) -> (R, 1024)."""
    return run(state, pooled, HEAD_CHILDREN, 14, stages).mean(3).mean(2)
