"""Drop-in nn.Module surface of the reference's SA U-Net (Unet-SpatialAttention.py:41-163).

Same class names, constructor signatures, attribute tree and state_dict as the reference's `DoubleConv`,
`SpatialAttention` and `UNet`, registered in the reference's order (so a given torch.manual_seed gives the same initial
weights). `forward` runs the HIP kernels: the encoder, decoder, max-pool, transposed convs and outc are those of
`modules.UNet(use_se=False)`, and each skip-concat goes through csrc/spatial_attn.hip before its decoder block.
There is no CPU or eager fallback.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _lib, modules
from .engine import Act, Ctx, GradSink, SAUnit, pack_input, unpack_output
from .modules import MaxPool2d, _Lease, _PlanCache, _require_device, _resolve_dtype


class DoubleConv(modules.DoubleConv):
    """(Conv3x3 -> BN -> ReLU) x 2 without SE (Unet-SpatialAttention.py:41-56)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__(in_channels, out_channels, use_se=False)


class _SAPlan:
    """Stand-alone SpatialAttention on an NCHW tensor: buffers for one (B, C, H, W, dtype)."""

    def __init__(self, mod, B, Cn, H, W, dtype, device):
        ctx = self.ctx = Ctx(device, dtype)
        if Cn % 8:
            raise _lib.InsarError(f"SpatialAttention: {Cn} channels; the HIP path needs a multiple of 8")
        self.x = Act.alloc(B, H, W, Cn, dtype, device)
        self.out = Act.alloc(B, H, W, Cn, dtype, device)
        self.dout = Act.alloc(B, H, W, Cn, dtype, device)
        self.unit = SAUnit(ctx, mod, self.x, self.out, "SpatialAttention")
        self.params = self.unit.params()
        self.sink = GradSink(ctx, self.params)
        self.busy = False
        self.training = True

    def forward(self, x, training):
        self.training = training
        pack_input(x, self.x)
        self.unit.forward(training)
        return unpack_output(self.out)

    def backward(self, g):
        self.sink.select()
        pack_input(g, self.dout)
        self.unit.backward(self.dout, self.sink, self.training)
        return unpack_output(self.dout), [self.sink.view(p) for p in self.params]


class _SAFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, training, track, x, *params):
        out = plan.forward(x, training)
        ctx.plan = plan
        ctx.lease = _Lease(plan) if track else None
        return out

    @staticmethod
    def backward(ctx, g):
        dx, grads = ctx.plan.backward(g.contiguous())
        if ctx.lease:
            ctx.lease.release()
        return (None, None, None, dx) + tuple(grads)


class SpatialAttention(nn.Module):
    """out = x * sigmoid(DoubleConv(2, 1)(cat(mean_c x, max_c x))) (Unet-SpatialAttention.py:59-82). The arg-max of the
    channel maximum is the first channel that holds it, as torch.max(dim=1) returns; only that channel gets its gradient."""

    def __init__(self):
        super().__init__()
        self.compress_and_map = DoubleConv(2, 1)
        self.sigmoid = nn.Sigmoid()
        self.compute_dtype: Optional[torch.dtype] = None
        self._plans = _PlanCache()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _require_device(x, "SpatialAttention")
        b, c, h, w = x.shape
        dt = _resolve_dtype(self)
        plan = self._plans.get((b, c, h, w, dt, x.device), lambda: _SAPlan(self, b, c, h, w, dt, x.device))
        return _SAFn.apply(plan, self.training, torch.is_grad_enabled(), x, *plan.params)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._plans.clear()          # cached plans hold raw parameter pointers
        return out


class UNet(modules.UNet):
    """U-Net with spatial attention on the four skip-concats (Unet-SpatialAttention.py:85-163).

    forward(x: [B, in_channels, H, W]) -> logits [B, num_classes, H, W] (float32, NCHW); `compute_dtype` as in
    `modules.UNet`. Everything but the four `sa*` units is the plan of `modules.UNet(use_se=False)` (engine.UNetPlan)."""

    spatial_attention = True           # engine.UNetPlan / engine.grad_groups: run and group the sa{i} units

    def __init__(self, in_channels: int = 1, num_classes: int = 2, compute_dtype: Optional[torch.dtype] = None):
        nn.Module.__init__(self)
        self.inc = DoubleConv(in_channels, 64)
        self.down1 = nn.Sequential(MaxPool2d(2), DoubleConv(64, 128))
        self.down2 = nn.Sequential(MaxPool2d(2), DoubleConv(128, 256))
        self.down3 = nn.Sequential(MaxPool2d(2), DoubleConv(256, 512))
        self.down4 = nn.Sequential(MaxPool2d(2), DoubleConv(512, 1024))
        self.up1 = nn.ConvTranspose2d(1024, 512, kernel_size=2, stride=2)
        self.conv1 = DoubleConv(1024, 512)
        self.up2 = nn.ConvTranspose2d(512, 256, kernel_size=2, stride=2)
        self.conv2 = DoubleConv(512, 256)
        self.up3 = nn.ConvTranspose2d(256, 128, kernel_size=2, stride=2)
        self.conv3 = DoubleConv(256, 128)
        self.up4 = nn.ConvTranspose2d(128, 64, kernel_size=2, stride=2)
        self.conv4 = DoubleConv(128, 64)
        self.sa1 = SpatialAttention()
        self.sa2 = SpatialAttention()
        self.sa3 = SpatialAttention()
        self.sa4 = SpatialAttention()
        self.outc = nn.Conv2d(64, num_classes, kernel_size=1)
        self.compute_dtype = compute_dtype
        self._plans = _PlanCache()
        self._hooks: dict = {}
        self.per_stage_param_waits = True
