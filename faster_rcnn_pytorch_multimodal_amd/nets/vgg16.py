"""VGG16 detector - counterpart of the reference's lib/nets/vgg16.py (``--net vgg16``): inference, and training behind
``cfg.TRAIN.VGG16_EN``.

Body (vgg16.py:34-47): torchvision's ``vgg16()`` - ``features`` is configuration 'D' (13 convolutions 3x3 / pad 1 with a
bias, each followed by ``ReLU(inplace=True)``, and five ``MaxPool2d(2, 2)``), ``classifier`` is Linear(25088, 4096), ReLU,
Dropout, Linear(4096, 4096), ReLU, Dropout with fc8 removed.  torchvision is not a dependency of this package: the module
tree is restated here from its published configuration with plain ``nn`` modules, so that the state-dict keys
(``vgg.features.N.{weight,bias}``, ``vgg.classifier.{0,3}.{weight,bias}``) and shapes are torchvision's - PARITY UNPINNED
against torchvision (no torchvision output has been compared).  ``_layers['head']`` is ``features[:-1]``: the last pool is
not used, so the stride is 16 and net_conv has 512 channels.  fc7 = classifier(pool5.view(R, -1)), (R, 4096).

The ``nn`` modules under ``self.vgg`` own the parameters only; the forward walks them on NHWC tensors: every convolution is
a ``hip_modules.conv_bn_act`` GEMM with the bias and the ReLU in its epilogue (``features.0`` reads the image padded to 4
channels), every pool ``ops.maxpool2x2s2_nhwc``.  fc6 and fc7 are 1x1 convolutions over R "pixels" through
``hip_modules.conv_forward`` (so they follow cfg.TEST.CONV_BF16 / CONV_SPLIT_BF16 like every inference convolution); fc6 reads
the NHWC flattening of pool5, its filter's columns permuted once from the (C,7,7) order of the reference's ``view`` (cached,
storage-stable, refreshed after a weight change).  Both dropouts are the identity in eval mode.

Training is opt-in: ``cfg.TRAIN.VGG16_EN`` (default False).  While it is off a forward with ``mode != 'TEST'`` raises as an
inference-only net does.  With it on, ``features[0..9]`` - frozen by the reference (vgg16.py:41-43) - run as in inference under
``no_grad`` and the path is differentiable from ``features.10`` on: seven convolutions are ``conv_bn_act_train`` nodes, the two
in front of a pool (``features.14``, ``features.21``) run conv + bias + ReLU + pool as ONE node whose backward is
``maxpool2x2s2_bwd(relu=True)`` - the pool's gradient kernel writes the gradient of the convolution's raw output, no
``act_bwd`` pass over the full-size map - and conv3_1's input takes no gradient, so no data gradient is launched for it.
fc6 and fc7 are ``linear_train`` nodes, each followed by its ``nn.Dropout`` (the reference has no ``train()`` override: both
are live with p = 0.5 after ``net.train()``) as a counter-based mask (``frcnn_dropout_fwd / _bwd``, stream ids
``DROPOUT_STREAM``, seeds from ``Network.uc_seed_args``: a captured step reads its seed from a device word that the runner
rewrites before every replay).  fc6 reads the NCHW flattening of pool5 (``FC6_NCHW_FLATTEN``, a 26 MB copy at 256 RoIs) so that
its 411 MB filter gradient is added into ``param.grad`` in place; the permuted-filter route of inference costs a 411 MB
temporary, a 411 MB permute copy and a 411 MB ``add_`` per captured step (measured: 2.9 ms against 2.6 ms per tail forward +
backward, 849 MB against 464 MB of temporaries, profiles/vgg16_train.md).
Not built, each a ``NotImplementedError``: training ``features[0..9]`` (the stem reads the image padded to 4 channels), a live
classifier Dropout during a ``TEST`` forward, FPN, the custom tail and the UC flags.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import ops
from ..model.config import cfg
from ..utils.init_utils import normal_init
from .autograd_ops import (_DropoutFn, _PermutedLinearFn, conv_bn_act_train, conv_relu_pool_train, linear_train,
                           maxpool2x2_train)
from .hip_modules import conv_bn_act, conv_forward, to_nchw_view, to_nhwc
from .network import Network

# torchvision's configuration 'D'
CFG_D = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M')
FIXED_CHILDREN = 10          # features[0..9] (conv1_x, conv2_x and their pools) stay frozen (vgg16.py:41-43)
POOLED = 7                   # the classifier reads (512, 7, 7) RoI features
# counter-based draws (csrc/rng.h) of the classifier's two dropouts in a training step - listed here once; distinct from
# uncertainty.STREAM (11..16) and ops.AUG_STREAM
DROPOUT_STREAM = {'fc6_drop': 21, 'fc7_drop': 22}
# Training: fc6 reads pool5 flattened in NCHW order - the reference's ``view`` - through plain ``linear_train``, whose filter
# gradient adds into param.grad in place.  False (A/B, tools/vgg16_train_bench.py): the NHWC flattening against the permuted
# filter (``_PermutedLinearFn``), whose gradient goes through a temporary, a permute copy and an add_.
FC6_NCHW_FLATTEN = True
NOT_BUILT = ("the 2x2 max-pool's backward kernel and the classifier's dropout in a training step are not built into a net "
             "while cfg.TRAIN.VGG16_EN is False (set it to train features[10..], fc6 and fc7)")
STEM_NOT_TRAINABLE = ("a parameter of vgg.features[0..%d] requires a gradient: conv1_x / conv2_x cannot train on the HIP path - "
                      "the reference freezes them (vgg16.py:41-43) and features.0 reads the 3-channel image padded to 4 "
                      "channels, which the differentiable convolution does not take" % (FIXED_CHILDREN - 1))


def train_enabled():
    return bool(cfg.TRAIN.get('VGG16_EN', False))


def vgg16_modules():
    """torchvision's ``vgg16()`` with fc8 removed (vgg16.py:35-38): an ``nn.Module`` with ``features`` (31 children) and
    ``classifier`` (6 children), initialised as torchvision's constructor leaves it."""
    layers, cin = [], 3
    for v in CFG_D:
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    body = nn.Module()
    body.features = nn.Sequential(*layers)
    body.classifier = nn.Sequential(nn.Linear(512 * POOLED * POOLED, 4096), nn.ReLU(True), nn.Dropout(),
                                    nn.Linear(4096, 4096), nn.ReLU(True), nn.Dropout())
    for m in body.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, 0, 0.01)
            nn.init.constant_(m.bias, 0)
    return body


class vgg16(Network):
    def __init__(self):
        Network.__init__(self)
        if cfg.ENABLE_CUSTOM_TAIL:
            raise NotImplementedError("cfg.ENABLE_CUSTOM_TAIL: the VGG16 tail is the body's own classifier (fc6, fc7)")
        if cfg.USE_FPN:
            raise NotImplementedError("cfg.USE_FPN: the reference builds no pyramid on VGG16")
        uc = [k for k in cfg.UC if k.startswith('EN_') and cfg.UC[k]]
        if uc:
            raise NotImplementedError("cfg.UC.%s: the uncertainty heads are built for the ResNet and LiDAR detectors only"
                                      % ", cfg.UC.".join(uc))
        self._feat_stride = 16
        self._fpn_en = False
        self._net_conv_channels = 512
        self._roi_pooling_channels = 512
        self._fc7_channels = 4096
        self._det_net_channels = 4096

    def init_weights(self):
        # the body keeps torchvision's initialisation (vgg16_modules); RPN and heads as the other image backbones
        normal_init(self.rpn_net, 0, 0.01, cfg.TRAIN.TRUNCATED)
        normal_init(self.rpn_cls_score_net, 0, 0.01, cfg.TRAIN.TRUNCATED)
        normal_init(self.rpn_bbox_pred_net, 0, 0.01, cfg.TRAIN.TRUNCATED)
        normal_init(self.cls_score_net, 0, 0.01, cfg.TRAIN.TRUNCATED)
        normal_init(self.bbox_pred_net, 0, 0.001, cfg.TRAIN.TRUNCATED)

    def _init_head_tail(self):
        # vgg16.py:34-47
        self.vgg = vgg16_modules()
        for layer in range(FIXED_CHILDREN):
            for p in self.vgg.features[layer].parameters():
                p.requires_grad = False
        self._layers['head'] = nn.Sequential(*list(self.vgg.features.children())[:-1])      # not using the last maxpool

    def key_transform(self, key):
        # vgg16.py:61-70
        return key if 'features.' in key else None

    def load_trimmed_pretrained_cnn(self, state_dict):
        # vgg16.py:72-81, without the print
        trimmed = OrderedDict()
        for key, param in state_dict.items():
            new_key = self.key_transform(key)
            if new_key is not None:
                trimmed[new_key] = param
        self.load_pretrained_cnn(trimmed)

    def load_pretrained_cnn(self, state_dict):
        # vgg16.py:84-88 keeps the keys the body has.  strict=False: the trimmed dictionary carries no classifier.* key, and
        # the classifier is to stay as it was (a strict load of the reference's line raises on the missing keys)
        own = self.vgg.state_dict()
        self.vgg.load_state_dict({k: v for k, v in state_dict.items() if k in own}, strict=False)

    def forward(self, image, info, gt_boxes=None, gt_boxes_dc=None, mode='TRAIN'):
        if mode != 'TEST':
            if not train_enabled():
                raise NotImplementedError("vgg16.forward(mode=%r): inference only - %s" % (mode, NOT_BUILT))
            if any(p.requires_grad for m in list(self.vgg.features)[:FIXED_CHILDREN] for p in m.parameters()):
                raise NotImplementedError(STEM_NOT_TRAINABLE)
        return Network.forward(self, image, info, gt_boxes, gt_boxes_dc, mode=mode)

    def _training_pass(self):
        return getattr(self, '_mode', 'TEST') == 'TRAIN' and torch.is_grad_enabled() and train_enabled()

    def _live_dropouts(self):
        return [m for m in self.vgg.classifier if isinstance(m, nn.Dropout) and m.training and m.p > 0]

    def draws_step_randoms(self):
        # a training step draws the masks of the classifier's live dropouts
        return train_enabled() and bool(self._live_dropouts())

    def _image_to_head(self):
        self._pyramid = None
        x = to_nhwc(self._image)
        mods = list(self._layers['head'])
        train = self._training_pass()
        if train and any(p.requires_grad for m in mods[:FIXED_CHILDREN] for p in m.parameters()):
            raise NotImplementedError(STEM_NOT_TRAINABLE)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Conv2d):
                if train and i >= FIXED_CHILDREN and (x.requires_grad or any(p.requires_grad for p in m.parameters())):
                    if i + 2 < len(mods) and isinstance(mods[i + 2], nn.MaxPool2d):
                        x = conv_relu_pool_train(x, m)         # conv + bias + ReLU + pool: one node, no act_bwd in its backward
                        i += 3
                        continue
                    x = conv_bn_act_train(x, m, None, relu=True)
                else:
                    with torch.no_grad():
                        x = conv_bn_act(x, m, None, relu=True)     # the bias and the following ReLU run in the GEMM's epilogue
            elif isinstance(m, nn.MaxPool2d):
                x = maxpool2x2_train(x) if train and x.requires_grad else ops.maxpool2x2s2_nhwc(x)
            i += 1
        self._act_summaries['conv'] = x
        return to_nchw_view(x)

    _input_to_head = _image_to_head

    def _head_to_tail(self, pool5):
        fc6, _, drop6, fc7, _, drop7 = self.vgg.classifier
        if getattr(self, '_mode', 'TEST') != 'TEST':
            if not train_enabled():
                raise NotImplementedError("vgg16._head_to_tail: inference only - the classifier's dropout in a training step "
                                          "is not built into a net while cfg.TRAIN.VGG16_EN is False")
            return self._tail_train(pool5)
        if drop6.training or drop7.training:
            raise NotImplementedError("vgg16._head_to_tail: a classifier Dropout is in train() mode - the dropout of fc6 / "
                                      "fc7 is built for training steps only (mode='TRAIN' with cfg.TRAIN.VGG16_EN); call "
                                      "net.eval()")
        x = to_nhwc(pool5)
        r, p, _, c = x.shape
        # pool5.view(R, -1) flattens (C,7,7); x is the (7,7,C) flattening: fc6's columns are permuted to match
        w6 = _PermutedLinearFn._prepared(fc6, c, p)
        h = conv_forward(x.reshape(r, 1, 1, p * p * c), w6, None, fc6.bias.detach(), None, fc6, relu=True)
        w7 = fc7.weight.detach().view(fc7.out_features, 1, 1, fc7.in_features)
        h = conv_forward(h, w7, None, fc7.bias.detach(), None, fc7, relu=True)
        return self._heads_on_fc7(h.view(r, -1))

    def _tail_train(self, pool5):
        """fc7 of a training step: relu(fc6) -> dropout -> relu(fc7) -> dropout, differentiable (vgg16.py:57-59)."""
        fc6, _, drop6, fc7, _, drop7 = self.vgg.classifier
        seed, seed_dev = self.uc_seed_args() if self._live_dropouts() else (0, None)

        def dropped(h, drop, stream):
            if drop.training and drop.p > 0:
                return _DropoutFn.apply(h, drop.p, seed, DROPOUT_STREAM[stream], seed_dev)
            return h

        r = pool5.shape[0]
        if FC6_NCHW_FLATTEN:
            # pool5 is an NCHW-shaped view of NHWC storage: the copy IS the reference's pool5.view(R, -1)
            h = linear_train(pool5.contiguous().view(r, -1), fc6, relu=True)
        else:
            x = to_nhwc(pool5)
            _, p, _, c = x.shape
            h = linear_train(x.reshape(r, p * p * c), fc6, relu=True, weight_nhwc_from=(c, p))
        h = dropped(h, drop6, 'fc6_drop')
        h = linear_train(h, fc7, relu=True)
        return dropped(h, drop7, 'fc7_drop')
