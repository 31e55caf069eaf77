"""FCN-ResNet50, plain and with SE-gated bottlenecks, on the HIP kernels: drop-ins for `FCN_SingleChannel`
(PSPNet.py:41-104) and `FCN_SingleChannel_SE` (PSPNet-ChannelAttention.py:57-203). Despite the scripts' names both
networks are torchvision's `fcn_resnet50`: the ResNet-50 backbone at output stride 8 (deeplab._Backbone), the
`FCNHead(2048, num_classes)` = 3x3 conv 2048 -> 512, BN, ReLU, Dropout(0.1), 1x1 conv with bias, and a bilinear resize to
the input size. The SE variant wraps each of the 16 bottlenecks in `BottleneckWithSE` (:83-126), whose `SEBlock` (:57-79)
gates the bn3 output before the residual add:

    out = relu(s * bn3(conv3(.)) + identity),   s = sigmoid(W2 relu(W1 mean_hw bn3(conv3(.))))

`forward` runs a plan of HIP launches (FCNPlan). The trunk is deeplab.ResNetTrunkPlan's, shared with DeepLabV3-CA: the stem
(deeplab.StemPlan), the residual blocks (deeplab.BottleneckPlan), dropout on the device-counter mask, the output conv, the
resize, the launch tapes. This module adds what is the FCNs' own: the SE blocks (SEBottleneckPlan: squeeze, excitation,
gated residual apply; backward through the per-image sums of the gated gradient) and the head on deeplab.ConvUnit.
No CPU or eager fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib
from ._lib import InsarSeFwd, call, ptr
from .deeplab import Bottleneck, BottleneckPlan, ConvUnit, ResNetTrunkPlan, _Backbone, _ResNetSegBase
from .engine import Act, Ctx, GradSink, OutConvPlan, bn_bwd_desc
from .modules import _require_device


# ------------------------------------------------------------------------------------------------------------
# module tree (the reference's and torchvision's names)
# ------------------------------------------------------------------------------------------------------------
class SEBlock(nn.Module):
    """Squeeze-and-Excitation block (PSPNet-ChannelAttention.py:57-79); its arithmetic runs in SEBottleneckPlan."""

    def __init__(self, channel: int, reduction: int = 16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(
            nn.Conv2d(channel, channel // reduction, 1, bias=False),
            nn.ReLU(inplace=True),
            nn.Conv2d(channel // reduction, channel, 1, bias=False),
            nn.Sigmoid())


class BottleneckWithSE(nn.Module):
    """A ResNet Bottleneck with an SEBlock between bn3 and the residual add (:83-126): takes over the wrapped block's modules."""

    def __init__(self, bottleneck: nn.Module):
        super().__init__()
        self.conv1 = bottleneck.conv1
        self.bn1 = bottleneck.bn1
        self.conv2 = bottleneck.conv2
        self.bn2 = bottleneck.bn2
        self.conv3 = bottleneck.conv3
        self.bn3 = bottleneck.bn3
        self.relu = bottleneck.relu
        self.downsample = bottleneck.downsample
        self.se_block = SEBlock(bottleneck.conv3.out_channels)


class FCNHead(nn.Sequential):
    """torchvision segmentation.fcn.FCNHead(in_channels, channels)."""

    def __init__(self, in_channels: int, channels: int):
        inter = in_channels // 4
        super().__init__(nn.Conv2d(in_channels, inter, 3, padding=1, bias=False), nn.BatchNorm2d(inter), nn.ReLU(),
                         nn.Dropout(0.1), nn.Conv2d(inter, channels, 1))


class _FCN(nn.Module):
    """fcn_resnet50(weights=None): backbone + FCNHead(2048, 21); no aux classifier."""

    def __init__(self):
        super().__init__()
        self.backbone = _Backbone()
        self.classifier = FCNHead(2048, 21)


def _one_channel_stem() -> nn.Conv2d:
    return nn.Conv2d(1, 64, kernel_size=(7, 7), stride=(2, 2), padding=(3, 3), bias=False)


class _FCNBase(_ResNetSegBase):
    """What the two wrappers add to deeplab._ResNetSegBase: the module tree, the input check, the gradient layout.

    Initialisation differs from the reference's call site in one respect: `fcn_resnet50(pretrained=False)` still loads
    ImageNet weights into the BACKBONE (torchvision's legacy `pretrained_backbone=True` default, a network fetch), while
    these classes start the backbone from torch's default (kaiming) initialisation. To start where the reference starts,
    load a ResNet-50 ImageNet state_dict with `load_backbone_state_dict` (conv1 is mean-reduced over its three input
    channels, the reference's own rule for pretrained stems). `pretrained=True` (the COCO-trained head, another fetch) is
    refused; a checkpoint of a reference model made that way loads through `load_state_dict`, which drops the
    `model.aux_classifier.*` entries such a model carries (the forward pass never uses them)."""

    # DataParallel(sync_bn=True) refuses these networks: their plan has no synchronised BatchNorm path
    sync_bn_unsupported = "the FCN plan has no synchronised BatchNorm path"

    def _setup(self, backbone: str, pretrained: bool, compute_dtype: Optional[torch.dtype]) -> None:
        super()._setup(backbone, pretrained, compute_dtype)
        self.model = _FCN()

    def grad_groups(self) -> List[List[nn.Parameter]]:
        """Parameters grouped by the backward stage that completes their gradients, in completion order: the head, then
        layer4 ... layer1 (blocks last to first; a block's se_block weights in its stage), the stem with layer1. The layout of
        the flat gradient buffer, the DP buckets and DataParallel(shard_optimizer=True)'s parameter buffer."""
        bb, head = self.model.backbone, self.model.classifier

        def block(m):
            ps = [m.conv1.weight, m.bn1.weight, m.bn1.bias, m.conv2.weight, m.bn2.weight, m.bn2.bias,
                  m.conv3.weight, m.bn3.weight, m.bn3.bias]
            if m.downsample is not None:
                ps += [m.downsample[0].weight, m.downsample[1].weight, m.downsample[1].bias]
            if isinstance(m, BottleneckWithSE):
                ps += [m.se_block.fc[0].weight, m.se_block.fc[2].weight]
            return ps

        groups = [[head[4].weight, head[4].bias, head[0].weight, head[1].weight, head[1].bias]]
        for li in (4, 3, 2, 1):
            groups.append([p for m in reversed(list(bb[f"layer{li}"])) for p in block(m)])
        groups[-1] += [bb["conv1"].weight, bb["bn1"].weight, bb["bn1"].bias]
        return groups

    def _check_input(self, x: torch.Tensor) -> None:
        name = type(self).__name__
        if x.dim() != 4 or x.size(1) != 1:
            raise ValueError(f"{name} expected input shape (B, 1, H, W), but got {x.shape}. Check DataLoader/Dataset.")
        _require_device(x, name)

    def _new_plan(self, B: int, H: int, W: int, dtype: torch.dtype, device: torch.device) -> "FCNPlan":
        return FCNPlan(self, B, H, W, dtype, device)


class FCN_SingleChannel(_FCNBase):
    """Same constructor, attribute names and state_dict as PSPNet.py:41-104 (326 entries); forward on HIP.
    Torch's RNG is consumed in the reference's order: backbone (with the dropped fc), FCNHead(2048, 21), the replacement
    head (:63), the one-channel stem (:70)."""

    def __init__(self, num_classes: int = 2, backbone: str = "resnet50", pretrained: bool = False,
                 compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self._setup(backbone, pretrained, compute_dtype)
        self.model.classifier = FCNHead(2048, num_classes)                # :63-64
        self.model.backbone["conv1"] = _one_channel_stem()                # :70-89


class FCN_SingleChannel_SE(_FCNBase):
    """Same constructor, attribute names and state_dict as PSPNet-ChannelAttention.py:131-203 (358 entries); forward on
    HIP. RNG order as the reference's: backbone, FCNHead(2048, 21), the stem (:152), the replacement head (:172), then the
    16 SEBlocks in layer order (:177-181)."""

    def __init__(self, num_classes: int = 2, backbone: str = "resnet50", pretrained: bool = False,
                 compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self._setup(backbone, pretrained, compute_dtype)
        self.model.backbone["conv1"] = _one_channel_stem()                # :151-169
        self.model.classifier = FCNHead(2048, num_classes)                # :172-173
        for name, module in self.model.backbone.named_children():         # :177-181
            if name.startswith("layer"):
                for i, block in enumerate(module):
                    if isinstance(block, Bottleneck):
                        module[i] = BottleneckWithSE(block)


# ------------------------------------------------------------------------------------------------------------
# plan
# ------------------------------------------------------------------------------------------------------------
class SEBottleneckPlan(BottleneckPlan):
    """BottleneckWithSE: the Bottleneck plan with the SE gate between bn3 and the residual add.

    forward:  conv3 + bn3 statistics (scale, shift) -> insar_se_squeeze (relu = 0: per-image, per-row-part sums of y)
              -> insar_se_excite (q = scale * mean_hw y + shift, s = sigmoid(W2 relu(W1 q)))
              -> insar_se_res_apply (out = relu(s * (y * scale + shift) + identity)).
    backward: g = dout * [out > 0] (the identity branch takes g as it is) -> insar_bnrelu_bwd_reduce (relu = 0: the
              per-image sums A = sum_hw g, S = sum_hw g * y) -> insar_bnse_bwd_coef (use_se: ds = scale S + shift A, the MLP
              backward, dW1 / dW2, dgamma / dbeta, k1 / k2, coefB = dq / HW) -> insar_bnrelu_bwd_apply (relu = 0:
              dy = scale (s g + coefB - k1 - xhat k2)).
    Of the Bottleneck plan's backward fusions, the ReLU mask applied by the consumer's dgrad GEMM (deeplab.GATE_FUSE) carries
    over; the consumer's epilogue sums of this block's conv3 gradient (`plain_for`) are switched off: they cover the whole
    batch and the SE backward needs them per image."""

    plain_sums = False

    def __init__(self, ctx: Ctx, mod: BottleneckWithSE, x: Act, name: str):
        super().__init__(ctx, mod, x, name)
        u3 = self.u3
        self.w1, self.w2 = mod.se_block.fc[0].weight, mod.se_block.fc[2].weight
        self.C, self.Cr = u3.cout, self.w1.shape[0]
        if tuple(self.w1.shape[1:]) != (self.C, 1, 1) or tuple(self.w2.shape) != (self.C, self.Cr, 1, 1):
            raise _lib.InsarError(f"{name}: SE weights do not match C = {self.C}")
        B = x.B
        self.se_part = ctx.f32(B * u3.red_rows, 2, self.C)          # per image: u3.red_rows row parts of u3.red_rpp rows
        self.pooled, self.sq, self.gate = ctx.f32(B, 2, self.C), ctx.f32(B, self.C), ctx.f32(B, self.C)
        self.hid = ctx.f32(B, self.Cr)
        self.coefB = ctx.f32(B, self.C)
        self.se_ws = ctx.f32(B * (3 * self.C + self.Cr))

    def params(self):
        return super().params() + [self.w1, self.w2]

    def forward(self, training: bool) -> None:
        u3, s = self.u3, _lib.stream_ptr()
        self.u1.forward(training)
        self.u2.forward(training)
        if self.ud is not None:
            self.ud.forward(training)
        u3.forward(training, apply=False)
        call("insar_se_squeeze", u3.y.ref, ptr(u3.scale), ptr(u3.shift), ptr(self.se_part), 0, u3.red_rpp, s)
        d = InsarSeFwd()
        d.part, d.B, d.H, d.W, d.C, d.Cr, d.rows = ptr(self.se_part), u3.x.B, u3.Ho, u3.Wo, self.C, self.Cr, u3.red_rows
        d.scale, d.shift, d.w1, d.w2 = ptr(u3.scale), ptr(u3.shift), ptr(self.w1), ptr(self.w2)
        d.pooled, d.sq, d.hid, d.gate = ptr(self.pooled), ptr(self.sq), ptr(self.hid), ptr(self.gate)
        call("insar_se_excite", C.byref(d), s)
        call("insar_se_res_apply", u3.y.ref, ptr(u3.scale), ptr(u3.shift), ptr(self.gate), u3.res.ref, u3.out.ref, s)

    def _tail_backward(self, g: Act, sink: GradSink, training: bool) -> None:
        u3, ctx, s = self.u3, self.ctx, _lib.stream_ptr()
        if u3.dy is None:
            u3.dy = Act.alloc(u3.x.B, u3.Ho, u3.Wo, u3.cout, ctx.dtype, ctx.device)
        u3.bred_ready = False
        call("insar_bnrelu_bwd_reduce", g.ref, u3.y.ref, ptr(u3.scale), ptr(u3.shift), ptr(u3.red_part), 0, u3.red_rpp, s)
        d = bn_bwd_desc(u3.x.B, u3.Ho, u3.Wo, self.C, u3.bn, sink, u3.mean, u3.invstd, u3.k1, u3.k2)
        d.Cr, d.use_se = self.Cr, 1
        d.pooled, d.sq, d.hid, d.gate = ptr(self.pooled), ptr(self.sq), ptr(self.hid), ptr(self.gate)
        d.w1, d.w2 = ptr(self.w1), ptr(self.w2)
        d.dw1, d.dw2 = ptr(sink.view(self.w1)), ptr(sink.view(self.w2))
        d.coefB = ptr(self.coefB)
        call("insar_bnse_bwd_coef", C.byref(d), ptr(u3.red_part), u3.red_rows, ptr(u3.scale), ptr(u3.shift), ptr(self.se_ws),
             0, int(training), s)
        call("insar_bnrelu_bwd_apply", g.ref, u3.y.ref, ptr(u3.scale), ptr(u3.shift), ptr(u3.mean), ptr(u3.invstd),
             ptr(self.gate), ptr(self.coefB), ptr(u3.k1), ptr(u3.k2), u3.dy.ref, 0, s)
        with ctx.side_stream():
            u3._weight_grad(sink.view(u3.conv.weight))
        u3._input_grad(self.dz2, None, bstat_for=self.u2)


class FCNPlan(ResNetTrunkPlan):
    """The head of the FCN wrappers on the trunk: FCNHead = 3x3 conv + BN + ReLU, Dropout(0.1); the SE variant's blocks run
    through SEBottleneckPlan."""

    def __init__(self, net: _FCNBase, B: int, H: int, W: int, dtype: torch.dtype, device: torch.device):
        super().__init__(net, B, H, W, dtype, device, "the FCN")
        head = net.model.classifier
        self.head = ConvUnit(self.ctx, head[0], head[1], self.x5, None, True, "classifier.0")
        self._dropout_setup(head[3].p, self.head.cout)
        self.outc = OutConvPlan(self.ctx, head[4], self.zdrop)
        self._finish(net.grad_groups(), [self.head])

    def _block_plan(self, mod: nn.Module) -> type:
        return SEBottleneckPlan if isinstance(mod, BottleneckWithSE) else BottleneckPlan

    def _after_replay(self) -> None:
        self.outc.x = self.zdrop if self.drop_active else self.head.out

    def _head_forward(self, training: bool) -> None:
        self.head.forward(training)
        self.outc.x = self._dropout_forward(self.head.out, training)

    def _head_backward(self, dz: Act, sink: GradSink, training: bool, on_bucket) -> None:
        self.head.backward(self._dropout_backward(dz), sink, training, self.blocks[-1].grad_out())
        if on_bucket is not None:
            on_bucket(self, ("head", 0))
