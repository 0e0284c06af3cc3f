"""MobileNet-v1 detector - counterpart of the reference's lib/nets/mobilenet_v1.py (``--net mobile``).

Body (mobilenet_v1.py:33-49, 107-132): ``Conv2d_0`` is a 3x3 / stride 2 / pad 1 convolution 3 -> 32 with BatchNorm and
ReLU6; ``Conv2d_1`` .. ``Conv2d_13`` are pairs of a ``depthwise`` 3x3 (groups == C, pad 1) and a ``pointwise`` 1x1
convolution, each with BatchNorm and ReLU6.  ``_layers['head']`` is children [:12] (stride 16, 512 channels),
``_layers['tail']`` children [12:] on the pooled (R,512,7,7) RoIs followed by ``.mean(3).mean(2)`` -> fc7 (R,1024)
(:226-235, 266-270).

The ``nn`` modules under ``self.mobilenet`` own the parameters only (state-dict keys and shapes equal the reference's);
the forward pass walks them on NHWC tensors: the stem and the pointwise convolutions are ``hip_modules.conv_bn_act``
GEMMs with the ReLU epilogue, the depthwise layers ``ops.depthwise_conv3x3_nhwc``.  ReLU6 = min(relu(t), 6): the GEMM
kernels apply the lower half, the upper clamp is applied by the reader of the value - the following depthwise layer
(``in_cap=6``), or one ``ops.clamp_max_`` behind ``Conv2d_11`` (net_conv: read by the RPN and the RoIAlign) and behind
``Conv2d_13`` (read by the spatial mean).

Training is opt-in: ``cfg.TRAIN.MOBILENET_EN`` (default False).  While it is off a ``mode='TRAIN'`` forward raises as an
inference-only net does.  With it on, children below ``cfg.MOBILENET.FIXED_LAYERS`` (1..12; the stem ``Conv2d_0`` cannot
train: its GEMM reads a 3-channel input padded to 4) keep the inference path and save nothing, and every other child is ONE
autograd node (``autograd_ops.separable_pair_train``): its backward is ``ops.act_bwd_cap`` (the pointwise ReLU6 mask), the
GEMM filter and data gradients of the pointwise layer, and ``ops.depthwise_conv3x3_bwd_weight / _bwd_data``, which apply
the depthwise ReLU6 mask as they load.  The upper clamps behind ``Conv2d_11`` and ``Conv2d_13`` run inside their nodes.
BatchNorm stays frozen and folded.  Eager and captured steps (``enable_train_graphs``) both work.
"""
import torch
import torch.nn as nn

from .. import ops
from ..model.config import cfg
from ..utils.init_utils import normal_init, set_bn_eval, set_bn_fix
from .autograd_ops import separable_pair_train, spatial_mean_train
from .hip_modules import conv_bn_act, prepared_depthwise, to_nchw_view, to_nhwc
from .network import Network

# (stride, depth) of Conv2d_0 and of the 13 depthwise-separable pairs (mobilenet_v1.py:33-49)
STEM = (2, 32)
PAIRS = ((1, 64), (2, 128), (1, 128), (2, 256), (1, 256), (2, 512), (1, 512), (1, 512), (1, 512), (1, 512), (1, 512),
         (1, 1024), (1, 1024))
HEAD_CHILDREN = 12           # children [:12] are the head, [12:] the tail (mobilenet_v1.py:267-270)
RELU6_CAP = 6.0


def _conv_bn_relu6(cin, cout, kernel, stride, groups=1):
    return nn.Sequential(nn.Conv2d(cin, cout, kernel, stride, (kernel - 1) // 2, groups=groups, bias=False),
                         nn.BatchNorm2d(cout), nn.ReLU6(inplace=True))


def mobilenet_v1_base():
    """The reference's ``mobilenet_v1_base()`` without arguments: same module tree, names and parameter shapes."""
    layers = [('Conv2d_0', _conv_bn_relu6(3, STEM[1], 3, STEM[0]))]
    cin = STEM[1]
    for i, (stride, depth) in enumerate(PAIRS, 1):
        pair = nn.Sequential()
        pair.add_module('depthwise', _conv_bn_relu6(cin, cin, 3, stride, groups=cin))
        pair.add_module('pointwise', _conv_bn_relu6(cin, depth, 1, 1))
        layers.append(('Conv2d_%d' % i, pair))
        cin = depth
    body = nn.Sequential()
    for name, m in layers:
        body.add_module(name, m)
    return body


def _is_conv(m):
    return m.__class__.__name__.find('Conv') != -1


def train_enabled():
    return bool(cfg.TRAIN.get('MOBILENET_EN', False))


def run_children(x, children, in_cap, train=False, finish=False):
    """Walk body children on an NHWC tensor.  ``in_cap``: the pending upper clamp of ``x`` (6 behind a GEMM convolution,
    inf for a finished tensor).  The result's upper clamp is PENDING when the last child ended in a GEMM convolution -
    all of them do - unless ``finish``: then the last child's ReLU6 is completed (in place).
    ``train``: a child with a trainable parameter, or behind one, runs as one autograd node; the others run the inference
    path and save nothing."""
    children = list(children)
    for i, child in enumerate(children):
        last = finish and i == len(children) - 1
        if hasattr(child, 'depthwise'):
            if train and (x.requires_grad or any(p.requires_grad for p in child.parameters())):
                x = separable_pair_train(x, child, in_cap, finish_cap=last)
                in_cap = RELU6_CAP
                continue
            conv, bn = child.depthwise[0], child.depthwise[1]
            if bn.training:
                raise NotImplementedError("BatchNorm in training mode (batch statistics) is not on the HIP path yet")
            w, scale, shift = prepared_depthwise(conv, bn)
            x = ops.depthwise_conv3x3_nhwc(x, w, scale, shift, stride=conv.stride[0], relu=True, in_cap=in_cap,
                                           out_cap=RELU6_CAP)
            x = conv_bn_act(x, child.pointwise[0], child.pointwise[1], relu=True)
        else:
            assert in_cap == float('inf'), "Conv2d_0 reads the image"
            if train and any(p.requires_grad for p in child.parameters()):
                raise NotImplementedError(STEM_NOT_TRAINABLE)
            x = conv_bn_act(x, child[0], child[1], relu=True)
        if last:
            x = ops.clamp_max_(x, RELU6_CAP)
        in_cap = RELU6_CAP
    return x


STEM_NOT_TRAINABLE = ("cfg.MOBILENET.FIXED_LAYERS = 0: the stem Conv2d_0 cannot train on the HIP path - its GEMM convolution "
                      "reads the 3-channel image padded to 4 channels, which the differentiable convolution does not take; "
                      "FIXED_LAYERS 1..12 are supported")


class mobilenetv1(Network):
    def __init__(self):
        Network.__init__(self)
        if float(cfg.MOBILENET.DEPTH_MULTIPLIER) != 1.0:
            raise NotImplementedError("cfg.MOBILENET.DEPTH_MULTIPLIER = %s: the reference stores the value and builds the "
                                      "full-width body regardless (mobilenet_v1.py:201,238); only 1.0 is accepted"
                                      % (cfg.MOBILENET.DEPTH_MULTIPLIER,))
        if cfg.ENABLE_CUSTOM_TAIL:
            raise NotImplementedError("cfg.ENABLE_CUSTOM_TAIL: the MobileNet tail is children [12:] of the body")
        if cfg.USE_FPN:
            raise NotImplementedError("cfg.USE_FPN: the reference builds no pyramid on MobileNet")
        uc = [k for k in cfg.UC if k.startswith('EN_') and cfg.UC[k]]
        if uc:
            raise NotImplementedError("cfg.UC.%s: the uncertainty heads are built for the ResNet and LiDAR detectors only"
                                      % ", cfg.UC.".join(uc))
        self._feat_stride = 16
        self._fpn_en = False
        self._depth_multiplier = cfg.MOBILENET.DEPTH_MULTIPLIER      # stored and never used, as in the reference
        self._net_conv_channels = 512
        self._roi_pooling_channels = 512
        self._fc7_channels = 1024
        self._det_net_channels = 1024

    def init_weights(self):
        # mobilenet_v1.py:205-224: every convolution of the body N(0, 0.09) truncated; no body convolution has a bias
        for m in self.mobilenet.modules():
            if _is_conv(m):
                m.weight.data.normal_().fmod_(2).mul_(0.09).add_(0)
        normal_init(self.rpn_net, 0, 0.01, cfg.TRAIN.TRUNCATED)
        normal_init(self.rpn_cls_score_net, 0, 0.01, cfg.TRAIN.TRUNCATED)
        normal_init(self.rpn_bbox_pred_net, 0, 0.01, cfg.TRAIN.TRUNCATED)
        normal_init(self.cls_score_net, 0, 0.01, cfg.TRAIN.TRUNCATED)
        normal_init(self.bbox_pred_net, 0, 0.001, cfg.TRAIN.TRUNCATED)

    def _init_head_tail(self):
        # mobilenet_v1.py:237-270
        self.mobilenet = mobilenet_v1_base()
        assert 0 <= cfg.MOBILENET.FIXED_LAYERS <= 12
        for m in list(self.mobilenet.children())[:cfg.MOBILENET.FIXED_LAYERS]:
            for p in m.parameters():
                p.requires_grad = False
        self.mobilenet.apply(set_bn_fix)
        for m in self.mobilenet.modules():
            if _is_conv(m):
                regularised = cfg.MOBILENET.REGU_DEPTH or m.groups == 1
                m.weight.weight_decay = cfg.MOBILENET.WEIGHT_DECAY if regularised else 0
        children = list(self.mobilenet.children())
        self._layers['head'] = nn.Sequential(*children[:HEAD_CHILDREN])
        self._layers['tail'] = nn.Sequential(*children[HEAD_CHILDREN:])

    def train(self, mode=True):
        # mobilenet_v1.py:272-287: the fixed layers and every BatchNorm stay in eval mode
        nn.Module.train(self, mode)
        if mode:
            for m in list(self.mobilenet.children())[:cfg.MOBILENET.FIXED_LAYERS]:
                m.eval()
            self.mobilenet.apply(set_bn_eval)
        return self

    def eval(self):
        return nn.Module.eval(self)

    def load_pretrained_cnn(self, state_dict):
        # mobilenet_v1.py:289-293
        self.mobilenet.load_state_dict({k: state_dict['features.' + k] for k in list(self.mobilenet.state_dict())
                                        if 'features.' + k in state_dict})

    def forward(self, image, info, gt_boxes=None, gt_boxes_dc=None, mode='TRAIN'):
        if mode != 'TEST':
            if not train_enabled():
                raise NotImplementedError("mobilenetv1.forward(mode=%r): inference only while cfg.TRAIN.MOBILENET_EN is False "
                                          "(set it to run the depthwise data and filter gradients and the ReLU6 masks)" % (mode,))
            if cfg.MOBILENET.FIXED_LAYERS < 1:
                raise NotImplementedError(STEM_NOT_TRAINABLE)
        return Network.forward(self, image, info, gt_boxes, gt_boxes_dc, mode=mode)

    def _image_to_head(self):
        self._pyramid = None
        # finish: Conv2d_11's ReLU6 is completed - the RPN and the RoIAlign read net_conv as it is
        net_conv = run_children(to_nhwc(self._image), self._layers['head'], float('inf'), train=self._training_pass(),
                                finish=True)
        self._act_summaries['conv'] = net_conv
        return to_nchw_view(net_conv)

    _input_to_head = _image_to_head

    def _head_to_tail(self, pool5):
        if getattr(self, '_mode', 'TEST') != 'TEST' and not train_enabled():
            raise NotImplementedError("mobilenetv1._head_to_tail: inference only while cfg.TRAIN.MOBILENET_EN is False")
        # finish: Conv2d_13's ReLU6 is completed in front of the mean
        x = run_children(to_nhwc(pool5), self._layers['tail'], float('inf'), train=self._training_pass(), finish=True)
        if self._training_pass():
            return spatial_mean_train(x)
        return self._fc7_from_layer4(x)                  # mean + detection tail

    def _training_pass(self):
        return getattr(self, '_mode', 'TEST') == 'TRAIN' and torch.is_grad_enabled() and train_enabled()
