"""VGG16 restated on the CPU with torch functional calls from torchvision's published configuration 'D' and the
reference's lib/nets/vgg16.py:34-59 (no module of the package, of the reference or of torchvision is used):
``features`` = 13 convolutions 3x3 / pad 1 with a bias, each followed by a ReLU, and 2x2 / stride 2 max-pools behind
convolutions 2, 4, 7, 10 and 13; the head is ``features[:-1]`` (the last pool is not used); ``classifier`` = Linear(25088,
4096), ReLU, Dropout, Linear(4096, 4096), ReLU, Dropout on ``pool5.view(R, -1)`` (eval mode: the dropouts are the identity).
Runs in fp32 and float64 and returns every stage.  Also the key / shape table and the seeded weight procedure of
tests/test_vgg16.py.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

CFG_D = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M')
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
POOL_INDEX = (4, 9, 16, 23, 30)
FROZEN_BELOW = 10
SEED = 20262


def key_shapes():
    """[(state-dict key under ``vgg.``, shape)] in module order."""
    out, cin, idx = [], 3, 0
    for v in CFG_D:
        if v == 'M':
            idx += 1
            continue
        out += [('features.%d.weight' % idx, (v, cin, 3, 3)), ('features.%d.bias' % idx, (v,))]
        cin, idx = v, idx + 2
    out += [('classifier.0.weight', (4096, 25088)), ('classifier.0.bias', (4096,)),
            ('classifier.3.weight', (4096, 4096)), ('classifier.3.bias', (4096,))]
    return out


def seeded_state(seed=SEED):
    """Weights from names and shapes alone: one numpy ``default_rng(seed)`` stream, tensors visited in SORTED key order;
    convolution and Linear weights N(0, sqrt(2 / fan_in)), biases U(-0.1, 0.1).  Drawn as fp32 - the values the device
    holds - so the float64 evaluation differs from the fp32 ones in its arithmetic only.  OrderedDict of fp32 tensors in
    module order."""
    rng = np.random.default_rng(seed)
    shapes = key_shapes()
    made = {}
    for key, shape in sorted(shapes):
        if key.endswith('.weight'):
            w = rng.standard_normal(shape, dtype=np.float32)
            w *= np.float32(np.sqrt(2.0 / float(np.prod(shape[1:]))))
            made[key] = w
        else:
            made[key] = rng.uniform(-0.1, 0.1, shape).astype(np.float32)
    return OrderedDict((k, torch.from_numpy(made[k])) for k, _ in shapes)


def head(state, x, stages=None):
    """``features[:-1]`` on the NCHW tensor ``x``; the weights are used in ``x``'s dtype.  ``stages``: a list that receives
    the output of every convolution (after its ReLU) and of every pool, 17 tensors; the last is net_conv."""
    idx = 0
    for v in CFG_D[:-1]:
        if v == 'M':
            x = F.max_pool2d(x, 2, 2)
            idx += 1
        else:
            x = F.relu(F.conv2d(x, state['features.%d.weight' % idx].to(x.dtype), state['features.%d.bias' % idx].to(x.dtype),
                                1, 1))
            idx += 2
        if stages is not None:
            stages.append(x)
    return x


def fc(state, index, x):
    """relu(classifier.<index>) on the (R, in_features) tensor ``x``."""
    return F.relu(F.linear(x, state['classifier.%d.weight' % index].to(x.dtype), state['classifier.%d.bias' % index].to(x.dtype)))


def tail(state, pooled, stages=None):
    """The classifier on the pooled (R,512,7,7) NCHW RoIs: fc7 (R, 4096).  ``stages`` receives fc6 and fc7."""
    fc6 = fc(state, 0, pooled.reshape(pooled.shape[0], -1))
    fc7 = fc(state, 3, fc6)
    if stages is not None:
        stages += [fc6, fc7]
    return fc7
