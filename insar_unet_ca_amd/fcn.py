"""FCN-ResNet50, plain and with SE-gated bottlenecks, on the HIP kernels: drop-ins for `FCN_SingleChannel`
(PSPNet.py:41-104) and `FCN_SingleChannel_SE` (PSPNet-ChannelAttention.py:57-203). Despite the scripts' names both
networks are torchvision's `fcn_resnet50`: the ResNet-50 backbone at output stride 8 (deeplab._Backbone), the
`FCNHead(2048, num_classes)` = 3x3 conv 2048 -> 512, BN, ReLU, Dropout(0.1), 1x1 conv with bias, and a bilinear resize to
the input size. The SE variant wraps each of the 16 bottlenecks in `BottleneckWithSE` (:83-126), whose `SEBlock` (:57-79)
gates the bn3 output before the residual add:

    out = relu(s * bn3(conv3(.)) + identity),   s = sigmoid(W2 relu(W1 mean_hw bn3(conv3(.))))

`forward` runs a plan of HIP launches (FCNPlan): the backbone's blocks as DeepLabV3-CA runs them (deeplab.BottleneckPlan),
the SE blocks through SEBottleneckPlan (squeeze, excitation, gated residual apply; backward through the per-image sums of
the gated gradient), the head on deeplab.ConvUnit, dropout on the device-counter mask, the output conv and the resize.
No CPU or eager fallback.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib, tape
from ._lib import InsarBnFinalize, InsarBnSeBwd, InsarSeFwd, call, ptr
from .deeplab import Bottleneck, BottleneckPlan, ConvUnit, _Backbone
from .engine import Act, Ctx, GradSink, OutConvPlan, WeightSet, _rows_per_part
from .modules import _PlanCache, _UNetFn, _require_device, _resolve_dtype
from .tape import tape_py


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


class _FCNBase(nn.Module):
    """What the two wrappers share: checks, checkpoint loading, forward on the HIP plan.

    Initialisation differs from the reference's call site in one respect: `fcn_resnet50(pretrained=False)` still loads
    ImageNet weights into the BACKBONE (torchvision's legacy `pretrained_backbone=True` default, a network fetch), while
    these classes start the backbone from torch's default (kaiming) initialisation. To start where the reference starts,
    load a ResNet-50 ImageNet state_dict with `load_backbone_state_dict` (conv1 is mean-reduced over its three input
    channels, the reference's own rule for pretrained stems). `pretrained=True` (the COCO-trained head, another fetch) is
    refused; a checkpoint of a reference model made that way loads through `load_state_dict`, which drops the
    `model.aux_classifier.*` entries such a model carries (the forward pass never uses them)."""

    # DataParallel(sync_bn=True) refuses these networks: their plan has no synchronised BatchNorm path
    sync_bn_unsupported = "the FCN plan has no synchronised BatchNorm path"

    def _setup(self, name: str, backbone: str, pretrained: bool, compute_dtype: Optional[torch.dtype]) -> None:
        if backbone != "resnet50":
            raise ValueError(f"Unsupported backbone: {backbone}" if backbone != "resnet101" else
                             "resnet101 is not part of BASELINE.json's configurations")
        if pretrained:
            raise _lib.InsarError("pretrained=True needs torchvision's downloaded weights; load a state_dict instead")
        self._name = name
        self.compute_dtype = compute_dtype
        self.model = _FCN()

    def _finish(self) -> None:
        self._plans = _PlanCache()
        self._hooks: dict = {}

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

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """As nn.Module.load_state_dict, except that `model.aux_classifier.*` keys are ignored."""
        if any(k.startswith("model.aux_classifier.") for k in state_dict):
            state_dict = OrderedDict((k, v) for k, v in state_dict.items() if not k.startswith("model.aux_classifier."))
        return super().load_state_dict(state_dict, strict=strict, **kw)

    @torch.no_grad()
    def load_backbone_state_dict(self, resnet_state_dict, strict: bool = True):
        """Load a torchvision ResNet-50 state_dict into the backbone: `fc.*` is dropped and a 3-channel `conv1.weight`
        becomes the 1-channel stem by averaging over its input channels."""
        sd = OrderedDict((k, v) for k, v in resnet_state_dict.items() if not k.startswith("fc."))
        w = sd.get("conv1.weight")
        if w is not None and w.shape[1] == 3:
            sd["conv1.weight"] = w.mean(dim=1, keepdim=True)
        if any(isinstance(m, BottleneckWithSE) for m in self.model.backbone.modules()):
            own = self.model.backbone.state_dict()
            missing = [k for k in own if ".se_block." in k]
            res = self.model.backbone.load_state_dict(sd, strict=False)
            bad = [k for k in res.missing_keys if k not in missing] + list(res.unexpected_keys)
            if strict and bad:
                raise RuntimeError(f"load_backbone_state_dict: mismatched keys {bad[:8]}")
            return res
        return self.model.backbone.load_state_dict(sd, strict=strict)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or x.size(1) != 1:
            raise ValueError(f"{self._name} expected input shape (B, 1, H, W), but got {x.shape}. Check DataLoader/Dataset.")
        _require_device(x, self._name)
        b, _c, h, w = x.shape
        dt = _resolve_dtype(self)
        plan = self._plans.get((b, h, w, dt, x.device), lambda: FCNPlan(self, b, h, w, dt, x.device))
        for bn in plan.bn_modules:
            if bn.training != self.training:
                raise _lib.InsarError(f"{self._name}: mixed BatchNorm modes are not supported by the HIP path")
        return _UNetFn.apply(plan, self.training, torch.is_grad_enabled(), self._hooks, x, *plan.grad_params)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if isinstance(getattr(self, "_plans", None), _PlanCache):
            self._plans.clear()
        return out


class FCN_SingleChannel(_FCNBase):
    """Same constructor, attribute names and state_dict as PSPNet.py:41-104 (326 entries); forward on HIP.
    Torch's RNG is consumed in the reference's order: backbone (with the dropped fc), FCNHead(2048, 21), the replacement
    head (:63), the one-channel stem (:70)."""

    def __init__(self, num_classes: int = 2, backbone: str = "resnet50", pretrained: bool = False,
                 compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self._setup("FCN_SingleChannel", backbone, pretrained, compute_dtype)
        self.model.classifier = FCNHead(2048, num_classes)                # :63-64
        self.model.backbone["conv1"] = _one_channel_stem()                # :70-89
        self._finish()


class FCN_SingleChannel_SE(_FCNBase):
    """Same constructor, attribute names and state_dict as PSPNet-ChannelAttention.py:131-203 (358 entries); forward on
    HIP. RNG order as the reference's: backbone, FCNHead(2048, 21), the stem (:152), the replacement head (:172), then the
    16 SEBlocks in layer order (:177-181)."""

    def __init__(self, num_classes: int = 2, backbone: str = "resnet50", pretrained: bool = False,
                 compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self._setup("FCN_SingleChannel_SE", backbone, pretrained, compute_dtype)
        self.model.backbone["conv1"] = _one_channel_stem()                # :151-169
        self.model.classifier = FCNHead(2048, num_classes)                # :172-173
        for name, module in self.model.backbone.named_children():         # :177-181
            if name.startswith("layer"):
                for i, block in enumerate(module):
                    if isinstance(block, Bottleneck):
                        module[i] = BottleneckWithSE(block)
        self._finish()


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
        d = InsarBnSeBwd()
        d.B, d.H, d.W, d.C, d.Cr, d.use_se = u3.x.B, u3.Ho, u3.Wo, self.C, self.Cr, 1
        d.mean, d.invstd = ptr(u3.mean), ptr(u3.invstd)
        d.pooled, d.sq, d.hid, d.gate = ptr(self.pooled), ptr(self.sq), ptr(self.hid), ptr(self.gate)
        d.w1, d.w2 = ptr(self.w1), ptr(self.w2)
        d.dw1, d.dw2 = ptr(sink.view(self.w1)), ptr(sink.view(self.w2))
        d.dgamma, d.dbeta = ptr(sink.view(u3.bn.weight)), ptr(sink.view(u3.bn.bias))
        d.coefB, d.k1, d.k2 = ptr(self.coefB), ptr(u3.k1), ptr(u3.k2)
        d.accumulate = 0
        call("insar_bnse_bwd_coef", C.byref(d), ptr(u3.red_part), u3.red_rows, ptr(u3.scale), ptr(u3.shift), ptr(self.se_ws),
             0, int(training), s)
        call("insar_bnrelu_bwd_apply", g.ref, u3.y.ref, ptr(u3.scale), ptr(u3.shift), ptr(u3.mean), ptr(u3.invstd),
             ptr(self.gate), ptr(self.coefB), ptr(u3.k1), ptr(u3.k2), u3.dy.ref, 0, s)
        with ctx.side_stream():
            u3._weight_grad(sink.view(u3.conv.weight))
        u3._input_grad(self.dz2, None, bstat_for=self.u2)


class FCNPlan(tape.PlanTape):
    """Buffers + launch sequence of the FCN wrappers' forward / backward for one input geometry. Stem and residual layers
    launch exactly as deeplab.DeepLabPlan's do (the plain blocks are the same BottleneckPlan)."""

    def __init__(self, net: _FCNBase, B: int, H: int, W: int, dtype: torch.dtype, device: torch.device):
        if H % 8 or W % 8:
            raise _lib.InsarError(f"H={H}, W={W}: the HIP path of the FCN covers inputs that are multiples of 8 (output stride 8)")
        self.net, self.B, self.H, self.W = net, B, H, W
        ctx = self.ctx = Ctx(device, dtype)
        A = lambda h, w, c: Act.alloc(B, h, w, c, dtype, device)
        bb, head = net.model.backbone, net.model.classifier
        # stem (as DeepLabPlan)
        self.stem_conv, self.stem_bn = bb["conv1"], bb["bn1"]
        h2, w2, h4, w4 = H // 2, W // 2, H // 4, W // 4
        self.y0, self.z0, self.p0 = A(h2, w2, 64), A(h2, w2, 64), A(h4, w4, 64)
        self.pool_arg = torch.zeros((B, h4, w4, 64), dtype=torch.uint8, device=device)
        self.st_rows = call("insar_conv7x7s2_fwd_rows", B, H)
        self.st_stats = ctx.f32(self.st_rows, 2, 64)
        self.st_rps = 0 if self.st_rows <= 256 else max(64, -(-self.st_rows // 64))
        self.st_fold = self.st_rows if not self.st_rps else -(-self.st_rows // self.st_rps)
        self.st_sums = ctx.f32(self.st_fold, 2, 64) if self.st_rps else self.st_stats
        self.st_scale, self.st_shift, self.st_mean, self.st_invstd, self.st_k1, self.st_k2 = (ctx.f32(64) for _ in range(6))
        self.st_rpp = _rows_per_part(B, h2)
        self.st_red_rows = -(-h2 // self.st_rpp)
        self.st_red = ctx.f32(B * self.st_red_rows, 2, 64)
        self.st_ws = ctx.f32(B * (3 * 64 + 1))
        self.st_nb = call("insar_conv7x7s2_wgrad_blocks", B, h2)
        self.st_part = ctx.f32(self.st_nb, 64 * 49)
        self.dz0 = self.dy0 = self.dp0 = None
        # residual layers
        self.blocks: List[BottleneckPlan] = []
        self.layer_blocks: List[List[BottleneckPlan]] = []
        x = self.p0
        for li in range(1, 5):
            grp = []
            for bi, mod in enumerate(bb[f"layer{li}"]):
                cls = SEBottleneckPlan if isinstance(mod, BottleneckWithSE) else BottleneckPlan
                blk = cls(ctx, mod, x, f"layer{li}.{bi}")
                grp.append(blk)
                self.blocks.append(blk)
                x = blk.out
            self.layer_blocks.append(grp)
        self.x5 = x
        h8, w8 = x.H, x.W
        # head: FCNHead = 3x3 conv + BN + ReLU, Dropout(0.1), 1x1 conv with bias; then the bilinear resize
        self.head = ConvUnit(ctx, head[0], head[1], self.x5, None, True, "classifier.0")
        self.drop_p = float(head[3].p)
        self.zdrop = A(h8, w8, self.head.cout)
        self.drop_mask = torch.zeros((B, h8, w8, self.head.cout), dtype=torch.uint8, device=device)
        self.drop_active = False
        self.drop_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.drop_counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.external_mask = False        # tests: apply a caller-supplied mask instead of drawing one
        self.outc = OutConvPlan(ctx, head[4], self.zdrop)
        self.K = head[4].out_channels
        self.logits_lo = None
        self._g = {}
        # parameters grouped by backward stage (completion order): head, layer4 ... layer1 + stem
        groups = net.grad_groups()
        self.grad_params = [p for g in groups for p in g]
        if len({id(p) for p in self.grad_params}) != len(list(net.parameters())) or len(self.grad_params) != len(list(net.parameters())):
            raise _lib.InsarError("FCNPlan: the gradient layout does not cover every parameter exactly once")
        self.sink = GradSink(ctx, None, groups)
        self.stage_sizes = self.sink.group_sizes
        self.stage_ends = [sum(self.stage_sizes[:i + 1]) for i in range(len(self.stage_sizes))]
        self._closes = {}
        self.units = [u for blk in self.blocks for u in blk.units()] + [self.head]
        self.weightset = WeightSet(ctx, [u.w for u in self.units])
        self.bn_modules = [self.stem_bn] + [u.bn for u in self.units]
        self._logits_lo = self._dlo = None
        self._tape_setup()
        self.busy = False
        self.training = True
        self.x_in: Optional[torch.Tensor] = None

    def bucket_closes(self, min_elems: int):
        if min_elems not in self._closes:
            from .parallel import plan_buckets
            self._closes[min_elems] = set(plan_buckets(self.stage_sizes, min_elems))
        return self._closes[min_elems]

    def _grad(self, key: str, like: Act) -> Act:
        if key not in self._g:
            self._g[key] = Act.alloc(like.B, like.H, like.W, like.c_len, like.buf.dtype, self.ctx.device)
        return self._g[key]

    def _tape_key(self, which: str) -> tuple:
        return super()._tape_key(which) + (self.drop_p,)

    # ---- forward -----------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, training: bool) -> torch.Tensor:
        """The ordinary launch sequence (_forward_eager) or, in the steady state of a training loop, its launch tape."""
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        if not self._tape_allowed(training, not self.external_mask):
            return self._forward_eager(x, training)
        logits = torch.empty((self.B, self.K, self.H, self.W), dtype=torch.float32, device=self.ctx.device)
        out, replayed = self._run(self._tape_key("f"), lambda: self._forward_eager(x, training),
                                  {"x": x.data_ptr(), "logits": logits.data_ptr()}, {x.data_ptr(): "x"},
                                  dyn_after=lambda o: {o.data_ptr(): "logits"})
        if replayed:
            self.training = training
            self.x_in = x.detach()
            self.drop_active = training and self.drop_p > 0.0
            self.outc.x = self.zdrop if self.drop_active else self.head.out
            return logits
        return out

    def _forward_eager(self, x: torch.Tensor, training: bool) -> torch.Tensor:
        s = _lib.stream_ptr()
        ctx = self.ctx
        self.training = training
        self.x_in = x.detach()
        with ctx.side_stream():
            self.weightset.refresh()
        # stem: conv7x7 s2 -> BN -> ReLU -> MaxPool(3, 2, 1)
        if training and self.B * (self.H // 2) * (self.W // 2) <= 1:
            raise ValueError("Expected more than 1 value per channel when training")
        call("insar_conv7x7s2_fwd", ptr(self.x_in), self.H, self.W, ptr(self.stem_conv.weight), self.y0.ref,
             ptr(self.st_stats) if training else 0, s)
        if training and self.st_rps:
            call("insar_colsum_partial", ptr(self.st_stats), ptr(self.st_sums), self.st_rows, 128, self.st_rps, s)
        bn = self.stem_bn
        d = InsarBnFinalize()
        d.part, d.rows, d.count, d.C, d.training = ptr(self.st_sums), self.st_fold, self.B * (self.H // 2) * (self.W // 2), 64, int(training)
        d.conv_bias = 0
        d.gamma, d.beta = ptr(bn.weight), ptr(bn.bias)
        d.running_mean, d.running_var, d.num_batches_tracked = ptr(bn.running_mean), ptr(bn.running_var), ptr(bn.num_batches_tracked)
        d.momentum, d.eps = (bn.momentum if bn.momentum is not None else 0.1), bn.eps
        d.scale, d.shift, d.mean, d.invstd = ptr(self.st_scale), ptr(self.st_shift), ptr(self.st_mean), ptr(self.st_invstd)
        call("insar_bn_finalize", C.byref(d), s)
        call("insar_bn_relu_apply", self.y0.ref, ptr(self.st_scale), ptr(self.st_shift), 0, self.z0.ref, 1, s)
        call("insar_maxpool3s2_fwd", self.z0.ref, self.p0.ref, ptr(self.pool_arg), s)
        ctx.join_side()                       # GEMM-layout weights are ready
        for blk in self.blocks:
            blk.forward(training)
        # head (FCNHead), dropout, output conv, resize to the input size
        self.head.forward(training)
        self.drop_active = training and self.drop_p > 0.0
        if self.drop_active:
            # mask = hash(seed drawn once from torch's RNG, device-side forward counter, element index): a new mask every
            # training forward, also when the step is replayed from a captured hipGraph
            ctr = self.drop_counter
            tape_py(lambda: ctr.add_(1))
            call("insar_dropout", self.head.out.ref, self.zdrop.ref, ptr(self.drop_mask), self.drop_seed, ptr(self.drop_counter),
                 self.drop_p, 0 if self.external_mask else 1, s)
            self.outc.x = self.zdrop
        else:
            self.outc.x = self.head.out
        z = self.head.out
        if self._logits_lo is None:
            self._logits_lo = torch.empty((self.B, self.K, z.H, z.W), dtype=torch.float32, device=ctx.device)
        self.logits_lo = self.outc.forward(out=self._logits_lo)
        logits = torch.empty((self.B, self.K, self.H, self.W), dtype=torch.float32, device=ctx.device)
        call("insar_bilinear_fwd", ptr(self.logits_lo), ptr(logits), self.B * self.K, z.H, z.W, self.H, self.W, s)
        return logits

    # ---- backward ------------------------------------------------------------------------------------------------
    def backward(self, dlogits: torch.Tensor, on_bucket=None) -> List[torch.Tensor]:
        if dlogits.dtype != torch.float32 or not dlogits.is_contiguous():
            dlogits = dlogits.float().contiguous()
        self.sink.select()
        if not self._tape_allowed(self.training, on_bucket is None and not self.external_mask and not self.weightset.stale()):
            return self._backward_eager(dlogits, on_bucket)
        xp = self.x_in.data_ptr()
        out, replayed = self._run(self._tape_key("b"), lambda: self._backward_eager(dlogits, None),
                                  {"dlogits": dlogits.data_ptr(), "x": xp}, {dlogits.data_ptr(): "dlogits", xp: "x"})
        if replayed:
            return [self.sink.view(p) for p in self.grad_params]
        return out

    def _backward_eager(self, dlogits: torch.Tensor, on_bucket=None) -> List[torch.Tensor]:
        s = _lib.stream_ptr()
        ctx, sink, training = self.ctx, self.sink, self.training
        z = self.head.out
        if self._dlo is None:
            self._dlo = torch.empty_like(self.logits_lo)
        dlo = self._dlo
        call("insar_bilinear_bwd", ptr(dlogits), ptr(dlo), self.B * self.K, z.H, z.W, self.H, self.W, s)
        dzo = self._grad("dzo", z)                       # gradient wrt the output conv's input
        self.outc.backward(dlo, sink, dzo)
        if self.drop_active:
            dz = self._grad("dz", z)
            call("insar_dropout", dzo.ref, dz.ref, ptr(self.drop_mask), 0, 0, self.drop_p, 0, s)
        else:
            dz = dzo
        self.head.backward(dz, sink, training, self.blocks[-1].grad_out())
        if on_bucket is not None:
            on_bucket(self, ("head", 0))
        # residual layers, last to first (as DeepLabPlan)
        if self.dp0 is None:
            self.dp0 = Act.alloc(self.p0.B, self.p0.H, self.p0.W, 64, ctx.dtype, ctx.device)
            self.dz0 = Act.alloc(self.z0.B, self.z0.H, self.z0.W, 64, ctx.dtype, ctx.device)
            self.dy0 = Act.alloc(self.z0.B, self.z0.H, self.z0.W, 64, ctx.dtype, ctx.device)
        for li in (3, 2, 1, 0):
            grp = self.layer_blocks[li]
            for bi in range(len(grp) - 1, -1, -1):
                blk = grp[bi]
                prev = grp[bi - 1] if bi > 0 else (self.layer_blocks[li - 1][-1] if li > 0 else None)
                dx = prev.grad_out() if prev is not None else self.dp0
                blk.backward(sink, training, dx, prev)
            if li > 0 and on_bucket is not None:
                on_bucket(self, ("layer", li + 1))
        # stem backward: MaxPool gradient, BN + ReLU backward, weight gradient of the 7x7 conv
        call("insar_maxpool3s2_bwd", self.dp0.ref, ptr(self.pool_arg), self.dz0.ref, s)
        call("insar_bnrelu_bwd_reduce", self.dz0.ref, self.y0.ref, ptr(self.st_scale), ptr(self.st_shift), ptr(self.st_red), 1,
             self.st_rpp, s)
        d = InsarBnSeBwd()
        d.B, d.H, d.W, d.C, d.Cr, d.use_se = self.B, self.z0.H, self.z0.W, 64, 1, 0
        d.mean, d.invstd = ptr(self.st_mean), ptr(self.st_invstd)
        d.dgamma, d.dbeta = ptr(sink.view(self.stem_bn.weight)), ptr(sink.view(self.stem_bn.bias))
        d.k1, d.k2 = ptr(self.st_k1), ptr(self.st_k2)
        d.accumulate = 0
        call("insar_bnse_bwd_coef", C.byref(d), ptr(self.st_red), self.st_red_rows, ptr(self.st_scale), ptr(self.st_shift),
             ptr(self.st_ws), 0, int(training), s)
        call("insar_bnrelu_bwd_apply", self.dz0.ref, self.y0.ref, ptr(self.st_scale), ptr(self.st_shift), ptr(self.st_mean),
             ptr(self.st_invstd), 0, 0, ptr(self.st_k1), ptr(self.st_k2), self.dy0.ref, 1, s)
        with ctx.side_stream():
            call("insar_conv7x7s2_wgrad", ptr(self.x_in), self.H, self.W, self.dy0.ref, ptr(self.st_part), _lib.stream_ptr())
            ctx.colsum(self.st_part, sink.view(self.stem_conv.weight).view(-1), 1, self.st_nb, 64 * 49)
        if on_bucket is not None:
            on_bucket(self, ("layer", 1))
        ctx.join_side()
        return [sink.view(p) for p in self.grad_params]
