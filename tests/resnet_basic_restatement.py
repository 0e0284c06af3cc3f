"""The BasicBlock ResNets (depth 18 / 34) restated on the CPU with plain ``torch.nn.functional`` calls from the reference's
lib/nets/resnet.py:34-71 (BasicBlock), :152-164 (stem and stages) and the published torchvision layout of ``resnet18`` /
``resnet34`` (no module of the package, of the reference or of torchvision is used):

    block(x)  = relu(bn2(conv2(relu(bn1(conv1(x))))) + identity),  conv1 3x3 / pad 1 / stride s, conv2 3x3 / pad 1 / stride 1,
                identity = x, or bn(conv1x1 / stride s (x)) where the block has a ``downsample``
    head      = conv1 7x7 / stride 2 / pad 3 + bn1 + relu, max-pool 3x3 / stride 2 / pad 1, layer1 (64), layer2 (128, stride 2),
                layer3 (256, stride 2): net_conv at stride 16 with 256 channels
    tail      = layer4 (512) on the pooled (R, 256, 7, 7) RoIs with layer4[0] at stride 1 (conv1 and the shortcut - the stated
                intent of resnet.py:235-238, which as written cannot run on a BasicBlock), then ``.mean(3).mean(2)``: fc7 (R, 512)

BatchNorm is evaluated in eval mode (running statistics).  Runs in fp32 and float64 and returns every stage.  Also the key /
shape table and the seeded weight procedure of tests/test_resnet_basic.py and tests/golden/make_golden_basicblock.py.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

LAYERS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}
PLANES = (64, 128, 256, 512)
SEED = 20341
EPS = 1e-5


def bn_shapes(prefix, c):
    return [(prefix + '.weight', (c,)), (prefix + '.bias', (c,)), (prefix + '.running_mean', (c,)),
            (prefix + '.running_var', (c,)), (prefix + '.num_batches_tracked', ())]


def block_shapes(prefix, inplanes, planes, down):
    """State-dict keys and shapes of one BasicBlock in module order; ``prefix`` ends with a dot or is empty."""
    out = [(prefix + 'conv1.weight', (planes, inplanes, 3, 3))] + bn_shapes(prefix + 'bn1', planes)
    out += [(prefix + 'conv2.weight', (planes, planes, 3, 3))] + bn_shapes(prefix + 'bn2', planes)
    if down:
        out += [(prefix + 'downsample.0.weight', (planes, inplanes, 1, 1))] + bn_shapes(prefix + 'downsample.1', planes)
    return out


def key_shapes(depth):
    """[(key, shape)] of torchvision's resnet18 / resnet34 without ``fc``, in module order."""
    out = [('conv1.weight', (64, 3, 7, 7))] + bn_shapes('bn1', 64)
    inplanes = 64
    for li, (planes, blocks) in enumerate(zip(PLANES, LAYERS[depth]), 1):
        for b in range(blocks):
            down = b == 0 and li > 1                              # stride 2 and a change of width; layer1 has neither
            out += block_shapes('layer%d.%d.' % (li, b), inplanes, planes, down)
            inplanes = planes
    return out


def seeded_from_shapes(shapes, seed=SEED):
    """Weights from names and shapes alone: one numpy ``default_rng(seed)`` stream, tensors visited in SORTED key order.
    Convolutions N(0, sqrt(2 / fan_in)); BatchNorm weight U(0.7, 0.9) - U(0.15, 0.25) for the bn2 that closes a residual branch,
    so that sixteen additions do not grow the maps -, bias and running_mean U(-0.1, 0.1), running_var U(0.8, 1.2),
    num_batches_tracked 0.  Drawn as fp32, the values the device holds.  OrderedDict of tensors in module order."""
    rng = np.random.default_rng(seed)
    made = {}
    for key, shape in sorted(shapes):
        if key.endswith('num_batches_tracked'):
            made[key] = np.zeros((), np.int64)
        elif key.endswith('running_var'):
            made[key] = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        elif key.endswith('running_mean') or key.endswith('.bias'):
            made[key] = rng.uniform(-0.1, 0.1, shape).astype(np.float32)
        elif len(shape) == 1:
            lo, hi = (0.15, 0.25) if '.bn2.' in key or key.startswith('bn2.') else (0.7, 0.9)
            made[key] = rng.uniform(lo, hi, shape).astype(np.float32)
        else:
            w = rng.standard_normal(shape, dtype=np.float32)
            w *= np.float32(np.sqrt(2.0 / float(np.prod(shape[1:]))))
            made[key] = w
    return OrderedDict((k, torch.from_numpy(np.asarray(made[k]))) for k, _ in shapes)


def seeded_state(depth, seed=SEED):
    return seeded_from_shapes(key_shapes(depth), seed)


def _bn(state, prefix, x):
    t = lambda name: state[prefix + '.' + name].to(x.dtype)
    return F.batch_norm(x, t('running_mean'), t('running_var'), t('weight'), t('bias'), False, 0.0, EPS)


def block(state, prefix, x, stride=1):
    """One BasicBlock on the NCHW tensor ``x``; the weights are used in ``x``'s dtype.  The shortcut is present iff the state
    has its keys."""
    out = F.relu(_bn(state, prefix + 'bn1', F.conv2d(x, state[prefix + 'conv1.weight'].to(x.dtype), None, stride, 1)))
    out = _bn(state, prefix + 'bn2', F.conv2d(out, state[prefix + 'conv2.weight'].to(x.dtype), None, 1, 1))
    identity = x
    if prefix + 'downsample.0.weight' in state:
        identity = _bn(state, prefix + 'downsample.1', F.conv2d(x, state[prefix + 'downsample.0.weight'].to(x.dtype), None, stride, 0))
    return F.relu(out + identity)


def stage(state, depth, li, x, first_stride):
    for b in range(LAYERS[depth][li - 1]):
        x = block(state, 'layer%d.%d.' % (li, b), x, first_stride if b == 0 else 1)
    return x


def head(state, depth, x, stages=None):
    """The stem and layer1 .. layer3 on the NCHW image ``x``.  ``stages`` receives the stem's output (behind the pool) and the
    three stage outputs; the last is net_conv."""
    x = F.relu(_bn(state, 'bn1', F.conv2d(x, state['conv1.weight'].to(x.dtype), None, 2, 3)))
    x = F.max_pool2d(x, 3, 2, 1)
    outs = [x]
    for li, stride in ((1, 1), (2, 2), (3, 2)):
        x = stage(state, depth, li, x, stride)
        outs.append(x)
    if stages is not None:
        stages += outs
    return x


def tail(state, depth, pooled, stages=None):
    """layer4 at stride 1 on the pooled (R,256,7,7) RoIs, then the spatial mean.  ``stages`` receives layer4's output
    (R,512,7,7) and fc7 (R,512)."""
    y = stage(state, depth, 4, pooled, 1)
    fc7 = y.mean(3).mean(2)
    if stages is not None:
        stages += [y, fc7]
    return fc7
