"""VGG16 detector - counterpart of the reference's lib/nets/vgg16.py (``--net vgg16``), inference.

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

Inference only: the pool has no backward kernel and the classifier's dropout is not built for a captured step, so a
forward with ``mode != 'TEST'`` raises.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import ops
from ..model.config import cfg
from ..utils.init_utils import normal_init
from .autograd_ops import _PermutedLinearFn
from .hip_modules import conv_bn_act, conv_forward, to_nchw_view, to_nhwc
from .network import Network

# torchvision's configuration 'D'
CFG_D = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M')
FIXED_CHILDREN = 10          # features[0..9] (conv1_x, conv2_x and their pools) stay frozen (vgg16.py:41-43)
POOLED = 7                   # the classifier reads (512, 7, 7) RoI features


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
            raise NotImplementedError("vgg16.forward(mode=%r): inference only - the 2x2 max-pool's backward kernel and the "
                                      "classifier's dropout in a training step are not built" % (mode,))
        return Network.forward(self, image, info, gt_boxes, gt_boxes_dc, mode=mode)

    def _image_to_head(self):
        self._pyramid = None
        x = to_nhwc(self._image)
        for m in self._layers['head']:
            if isinstance(m, nn.Conv2d):
                x = conv_bn_act(x, m, None, relu=True)         # the bias and the following ReLU run in the GEMM's epilogue
            elif isinstance(m, nn.MaxPool2d):
                x = ops.maxpool2x2s2_nhwc(x)
        self._act_summaries['conv'] = x
        return to_nchw_view(x)

    _input_to_head = _image_to_head

    def _head_to_tail(self, pool5):
        if getattr(self, '_mode', 'TEST') != 'TEST':
            raise NotImplementedError("vgg16._head_to_tail: inference only - the classifier's dropout in a training step "
                                      "is not built")
        fc6, _, drop6, fc7, _, drop7 = self.vgg.classifier
        if drop6.training or drop7.training:
            raise NotImplementedError("vgg16._head_to_tail: a classifier Dropout is in train() mode - the dropout of fc6 / "
                                      "fc7 is not built; call net.eval()")
        x = to_nhwc(pool5)
        r, p, _, c = x.shape
        # pool5.view(R, -1) flattens (C,7,7); x is the (7,7,C) flattening: fc6's columns are permuted to match
        w6 = _PermutedLinearFn._prepared(fc6, c, p)
        h = conv_forward(x.reshape(r, 1, 1, p * p * c), w6, None, fc6.bias.detach(), None, fc6, relu=True)
        w7 = fc7.weight.detach().view(fc7.out_features, 1, 1, fc7.in_features)
        h = conv_forward(h, w7, None, fc7.bias.detach(), None, fc7, relu=True)
        return self._heads_on_fc7(h.view(r, -1))
