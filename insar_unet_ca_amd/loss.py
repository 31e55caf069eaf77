"""Loss entry points of the training loop, on the HIP path.

`CrossEntropyLoss(ignore_index=255)` is the drop-in for the reference's criterion
(Unet-ChannalAttention.py:465, used at :344): mean over non-ignored pixels of
-log softmax(logits)[target]; forward and the gradient are produced by one fused pass.
`DiceLoss` / `DiceCELoss` are build-side additions (the reference has no Dice loss,
SURVEY §0): standard soft-Dice on softmax probabilities.

The imbalance-aware forms (csrc/loss_weighted.hip, DESIGN.md "Imbalance-aware losses"): `CrossEntropyLoss(weight=,
label_smoothing=)` with torch's semantics, `FocalLoss`, the same two inside `DiceCELoss`, and the helpers that produce the
weights: `label_histogram` (per-class pixel counts, accumulated on the device) and `class_weights` (host arithmetic).
"""
from __future__ import annotations

import math
import warnings

import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr


def _require_device(logits: torch.Tensor, who: str) -> None:
    if not logits.is_cuda:
        raise _lib.InsarError(f"{who}: logits are on {logits.device}; the HIP path needs a ROCm tensor (no CPU fallback)")


def _prep(logits: torch.Tensor, target: torch.Tensor, who: str):
    _require_device(logits, who)
    if logits.dim() < 2:
        raise _lib.InsarError(f"{who}: logits must be [B, K, ...]")
    B, K = logits.shape[0], logits.shape[1]
    HW = 1
    for d in logits.shape[2:]:
        HW *= d
    if target.shape != (B,) + tuple(logits.shape[2:]):
        raise _lib.InsarError(f"{who}: target shape {tuple(target.shape)} does not match logits {tuple(logits.shape)}")
    lg = logits.detach()
    if lg.dtype != torch.float32 or not lg.is_contiguous():
        lg = lg.float().contiguous()
    tg = target
    if tg.dtype != torch.int64 or not tg.is_contiguous():
        tg = tg.long().contiguous()
    return lg, tg, B, K, HW


def _scale_by(dl: torch.Tensor, g: torch.Tensor, in_dtype) -> torch.Tensor:
    """d loss / d logits times the incoming gradient of the scalar loss, on the HIP path (insar_mul_dev_f32: the factor is
    read from device memory; dl itself is kept for a second backward)."""
    if g.numel() != 1 or not g.is_cuda:
        # loss.backward(gradient=torch.tensor(2.0)) and the like: not the training loop's path, so plain torch arithmetic
        out = dl * g.detach().to(dl.device, dl.dtype)
        return out if in_dtype == torch.float32 else out.to(in_dtype)
    gs = g.detach()
    if gs.dtype != torch.float32:
        gs = gs.float()
    out = torch.empty_like(dl)
    call("insar_mul_dev_f32", ptr(out), ptr(dl), dl.numel(), ptr(gs), _lib.stream_ptr())
    return out if in_dtype == torch.float32 else out.to(in_dtype)


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        lg, tg, B, K, HW = _prep(logits, target, "CrossEntropyLoss")
        dl = torch.empty_like(lg)
        nb = call("insar_ce_blocks", B * HW)
        ws = torch.empty(2 + 2 * nb, dtype=torch.float32, device=lg.device)
        out = torch.empty(1, dtype=torch.float32, device=lg.device)
        call("insar_cross_entropy", ptr(lg), ptr(tg), B, K, HW, ignore_index, ptr(dl), ptr(out), ptr(ws), _lib.stream_ptr())
        ctx.dl = dl
        ctx.in_dtype = logits.dtype
        return out[0]

    @staticmethod
    def backward(ctx, g):
        return _scale_by(ctx.dl, g, ctx.in_dtype), None, None


class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, smooth):
        lg, tg, B, K, HW = _prep(logits, target, "DiceLoss")
        dl = torch.empty_like(lg)
        nb = call("insar_ce_blocks", B * HW)
        ws = torch.empty(3 * K * (nb + 1), dtype=torch.float32, device=lg.device)
        out = torch.empty(1, dtype=torch.float32, device=lg.device)
        call("insar_dice", ptr(lg), ptr(tg), B, K, HW, ignore_index, float(smooth), ptr(dl), ptr(out), ptr(ws),
             _lib.stream_ptr())
        ctx.dl = dl
        ctx.in_dtype = logits.dtype
        return out[0]

    @staticmethod
    def backward(ctx, g):
        return _scale_by(ctx.dl, g, ctx.in_dtype), None, None, None


class _DiceCEFn(torch.autograd.Function):
    """ce_weight*CE + dice_weight*Dice: one statistics pass and one gradient pass over the logits."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, smooth, ce_weight, dice_weight):
        lg, tg, B, K, HW = _prep(logits, target, "DiceCELoss")
        dl = torch.empty_like(lg)
        nb = call("insar_ce_blocks", B * HW)
        ws = torch.empty(3 + 3 * K + nb * (2 + 3 * K), dtype=torch.float32, device=lg.device)
        out = torch.empty(3, dtype=torch.float32, device=lg.device)
        call("insar_dice_ce", ptr(lg), ptr(tg), B, K, HW, ignore_index, float(smooth), float(ce_weight), float(dice_weight),
             ptr(dl), ptr(out), ptr(ws), _lib.stream_ptr())
        ctx.dl = dl
        ctx.in_dtype = logits.dtype
        ctx.parts = out           # [combined, ce, dice] for logging
        return out[0]

    @staticmethod
    def backward(ctx, g):
        return _scale_by(ctx.dl, g, ctx.in_dtype), None, None, None, None, None


class _CEWFn(torch.autograd.Function):
    """Class-weighted / label-smoothed CE (insar_cross_entropy_w): weight is a device float[K], read by the kernels."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, label_smoothing):
        lg, tg, B, K, HW = _prep(logits, target, "CrossEntropyLoss")
        dl = torch.empty_like(lg)
        nb = call("insar_ce_blocks", B * HW)
        ws = torch.empty(2 + 2 * nb, dtype=torch.float32, device=lg.device)
        out = torch.empty(1, dtype=torch.float32, device=lg.device)
        call("insar_cross_entropy_w", ptr(lg), ptr(tg), B, K, HW, ignore_index, ptr(weight), float(label_smoothing), ptr(dl),
             ptr(out), ptr(ws), _lib.stream_ptr())
        ctx.dl = dl
        ctx.in_dtype = logits.dtype
        return out[0]

    @staticmethod
    def backward(ctx, g):
        return _scale_by(ctx.dl, g, ctx.in_dtype), None, None, None, None


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, alpha, ignore_index, gamma):
        lg, tg, B, K, HW = _prep(logits, target, "FocalLoss")
        dl = torch.empty_like(lg)
        nb = call("insar_ce_blocks", B * HW)
        ws = torch.empty(2 + 2 * nb, dtype=torch.float32, device=lg.device)
        out = torch.empty(1, dtype=torch.float32, device=lg.device)
        call("insar_focal", ptr(lg), ptr(tg), B, K, HW, ignore_index, float(gamma), ptr(alpha), ptr(dl), ptr(out), ptr(ws),
             _lib.stream_ptr())
        ctx.dl = dl
        ctx.in_dtype = logits.dtype
        return out[0]

    @staticmethod
    def backward(ctx, g):
        return _scale_by(ctx.dl, g, ctx.in_dtype), None, None, None, None


class _DiceCEWFn(torch.autograd.Function):
    """ce_weight * (weighted / smoothed CE, or focal when focal_gamma >= 0) + dice_weight * Dice (insar_dice_ce_w)."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, smooth, ce_weight, dice_weight, label_smoothing, focal_gamma):
        lg, tg, B, K, HW = _prep(logits, target, "DiceCELoss")
        dl = torch.empty_like(lg)
        nb = call("insar_ce_blocks", B * HW)
        ws = torch.empty(4 + 3 * K + nb * (3 + 3 * K), dtype=torch.float32, device=lg.device)
        out = torch.empty(3, dtype=torch.float32, device=lg.device)
        call("insar_dice_ce_w", ptr(lg), ptr(tg), B, K, HW, ignore_index, float(smooth), float(ce_weight), float(dice_weight),
             ptr(weight), float(label_smoothing), float(focal_gamma), ptr(dl), ptr(out), ptr(ws), _lib.stream_ptr())
        ctx.dl = dl
        ctx.in_dtype = logits.dtype
        ctx.parts = out           # [combined, ce term, dice] for logging
        return out[0]

    @staticmethod
    def backward(ctx, g):
        return _scale_by(ctx.dl, g, ctx.in_dtype), None, None, None, None, None, None, None, None


MAX_CLASSES = 16          # LW_MAXK of csrc/loss_weighted.hip


def _class_vector(v, who: str, what: str) -> torch.Tensor:
    """A per-class vector (tensor, list or array) as a float32 1-D tensor of non-negative finite values."""
    t = v.detach().clone() if isinstance(v, torch.Tensor) else torch.as_tensor(v)
    if t.dim() != 1 or t.numel() < 1:
        raise _lib.InsarError(f"{who}: {what} must be a non-empty 1-D vector with one value per class, got shape {tuple(t.shape)}")
    if t.numel() > MAX_CLASSES:
        raise _lib.InsarError(f"{who}: {what} has {t.numel()} classes; the HIP path handles up to {MAX_CLASSES}")
    t = t.to(torch.float32).contiguous()
    if not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
        raise _lib.InsarError(f"{who}: {what} must be finite and non-negative, got {t.tolist()}")
    return t


def _check_smoothing(label_smoothing, who: str) -> float:
    ls = float(label_smoothing)
    if not (0.0 <= ls < 1.0):
        raise _lib.InsarError(f"{who}: label_smoothing={label_smoothing} must be in [0, 1)")
    return ls


def _vector_for(vec, logits: torch.Tensor, who: str, what: str):
    """The class vector as the kernels read it: length K, on the logits' device. None stays None."""
    if vec is None:
        return None
    K = logits.shape[1] if logits.dim() >= 2 else -1
    if vec.numel() != K:
        raise _lib.InsarError(f"{who}: {what} has {vec.numel()} entries but the logits have {K} classes")
    if vec.device != logits.device:
        raise _lib.InsarError(f"{who}: {what} is on {vec.device} but the logits are on {logits.device}; "
                              "move the criterion with .to(device)")
    if vec.dtype != torch.float32 or not vec.is_contiguous():
        # .double() / .half() / .to(dtype) on the criterion (or on a model that owns it) convert buffers; the kernels read float[K]
        raise _lib.InsarError(f"{who}: {what} is {vec.dtype}; the kernels read float32 (keep the criterion in float32: "
                              "criterion.float())")
    return vec


class CrossEntropyLoss(nn.Module):
    """Drop-in for nn.CrossEntropyLoss(weight=..., ignore_index=..., label_smoothing=...) with mean reduction and class-index
    targets. `weight` is a buffer named as torch's (state_dict key "weight", moved by .to())."""

    def __init__(self, weight=None, ignore_index: int = -100, reduction: str = "mean", label_smoothing: float = 0.0):
        super().__init__()
        if reduction != "mean":
            raise _lib.InsarError("CrossEntropyLoss HIP path: only reduction='mean'")
        self.label_smoothing = _check_smoothing(label_smoothing, "CrossEntropyLoss")
        self.register_buffer("weight", None if weight is None else _class_vector(weight, "CrossEntropyLoss", "weight"))
        # ones [K] for label smoothing without weights: made at the first call, kept (the same device pointer at every step),
        # not part of the state_dict
        self.register_buffer("_unit_weight", None, persistent=False)
        self.ignore_index = ignore_index

    def _ones(self, logits: torch.Tensor) -> torch.Tensor:
        u = self._unit_weight
        if u is None or u.numel() != logits.shape[1] or u.device != logits.device or u.dtype != torch.float32:
            self._unit_weight = u = torch.ones(logits.shape[1], dtype=torch.float32, device=logits.device)
        return u

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self.weight is None and self.label_smoothing == 0.0:
            return _CEFn.apply(logits, target, self.ignore_index)
        w = _vector_for(self.weight, logits, "CrossEntropyLoss", "weight")
        if w is None:
            _require_device(logits, "CrossEntropyLoss")
            if logits.dim() < 2:
                raise _lib.InsarError("CrossEntropyLoss: logits must be [B, K, ...]")
            w = self._ones(logits)
        return _CEWFn.apply(logits, target, w, self.ignore_index, self.label_smoothing)


class FocalLoss(nn.Module):
    """Multi-class focal loss on softmax probabilities: mean over valid pixels of alpha[y] (1 - p_y)^gamma (-log p_y).
    alpha: None, a per-class vector, or a float a meaning [1 - a, a] (the binary convention; two-class logits only).
    gamma = 0, alpha = None is CrossEntropyLoss."""

    def __init__(self, gamma: float = 2.0, alpha=None, ignore_index: int = 255):
        super().__init__()
        g = float(gamma)
        if not (0.0 <= g <= 64.0):
            raise _lib.InsarError(f"FocalLoss: gamma={gamma} must be in [0, 64]")
        self.gamma, self.ignore_index = g, ignore_index
        self.binary_alpha = isinstance(alpha, (int, float)) and not isinstance(alpha, bool)
        if self.binary_alpha:
            if not (0.0 <= float(alpha) <= 1.0):
                raise _lib.InsarError(f"FocalLoss: a scalar alpha must be in [0, 1], got {alpha}")
            alpha = [1.0 - float(alpha), float(alpha)]
        self.register_buffer("alpha", None if alpha is None else _class_vector(alpha, "FocalLoss", "alpha"))

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self.binary_alpha and (logits.dim() < 2 or logits.shape[1] != 2):
            raise _lib.InsarError(f"FocalLoss: a scalar alpha means [1 - a, a] for two classes; the logits have "
                                  f"{logits.shape[1] if logits.dim() >= 2 else '?'} (pass a per-class vector)")
        a = _vector_for(self.alpha, logits, "FocalLoss", "alpha")
        return _FocalFn.apply(logits, target, a, self.ignore_index, self.gamma)


class DiceLoss(nn.Module):
    """1 - mean_c (2*I_c + smooth) / (P_c + T_c + smooth) on softmax probabilities."""

    def __init__(self, ignore_index: int = 255, smooth: float = 1.0):
        super().__init__()
        self.ignore_index, self.smooth = ignore_index, smooth

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return _DiceFn.apply(logits, target, self.ignore_index, self.smooth)


class DiceCELoss(nn.Module):
    """ce_weight * CE + dice_weight * Dice (the 'Dice+CE' training objective of config 2). weight / label_smoothing act on
    the CE half as in CrossEntropyLoss; focal_gamma >= 0 replaces the CE half by FocalLoss(gamma, alpha=weight). Dice itself
    is never weighted."""

    def __init__(self, ignore_index: int = 255, smooth: float = 1.0, ce_weight: float = 1.0, dice_weight: float = 1.0,
                 weight=None, label_smoothing: float = 0.0, focal_gamma=None):
        super().__init__()
        self.ce = CrossEntropyLoss(weight=weight, ignore_index=ignore_index, label_smoothing=label_smoothing)
        self.dice = DiceLoss(ignore_index=ignore_index, smooth=smooth)
        self.ce_weight, self.dice_weight = ce_weight, dice_weight
        if focal_gamma is not None:
            if not (0.0 <= float(focal_gamma) <= 64.0):
                raise _lib.InsarError(f"DiceCELoss: focal_gamma={focal_gamma} must be None or in [0, 64]")
            if self.ce.label_smoothing != 0.0:
                raise _lib.InsarError("DiceCELoss: label_smoothing and focal_gamma do not combine")
        self.focal_gamma = None if focal_gamma is None else float(focal_gamma)

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self.ce.weight is None and self.ce.label_smoothing == 0.0 and self.focal_gamma is None:
            return _DiceCEFn.apply(logits, target, self.ce.ignore_index, self.dice.smooth, self.ce_weight, self.dice_weight)
        w = _vector_for(self.ce.weight, logits, "DiceCELoss", "weight")          # None: the kernels use ones
        return _DiceCEWFn.apply(logits, target, w, self.ce.ignore_index, self.dice.smooth, self.ce_weight, self.dice_weight,
                                self.ce.label_smoothing, -1.0 if self.focal_gamma is None else self.focal_gamma)


def label_histogram(masks_or_loader, num_classes: int, ignore_index: int = 255, device=None, return_ignored: bool = False):
    """Pixels per class of a mask tensor, or of every batch of a loader / list (items are masks, or tuples whose LAST element
    is the mask), counted by insar_label_hist and accumulated in device memory; read back once at the end.

    Returns an int64 CPU tensor [num_classes] (and the number of ignored pixels with return_ignored=True). Masks must be on
    the ROCm device, or `device` names the one to move them to. A label outside [0, num_classes) that is not ignore_index
    raises."""
    K = int(num_classes)
    if not (1 <= K <= MAX_CLASSES):
        raise _lib.InsarError(f"label_histogram: num_classes={num_classes} must be 1..{MAX_CLASSES}")
    batches = [masks_or_loader] if isinstance(masks_or_loader, torch.Tensor) else masks_or_loader
    counts, total = None, 0
    for item in batches:
        m = item if isinstance(item, torch.Tensor) else item[-1]
        if device is not None:
            m = m.to(device, non_blocking=True)
        if not m.is_cuda:
            raise _lib.InsarError(f"label_histogram: masks are on {m.device}; the HIP path needs a ROCm tensor "
                                  "(no CPU fallback; pass device=)")
        if m.dtype != torch.int64 or not m.is_contiguous():
            m = m.long().contiguous()
        if m.numel() == 0:
            continue
        if counts is None:
            counts = torch.zeros(K + 1, dtype=torch.int64, device=m.device)
        elif counts.device != m.device:
            raise _lib.InsarError(f"label_histogram: masks on {m.device} after masks on {counts.device}")
        nb = call("insar_ce_blocks", m.numel())
        ws = torch.empty((K + 1) * nb, dtype=torch.int64, device=m.device)
        call("insar_label_hist", ptr(m), m.numel(), K, ignore_index, ptr(counts), ptr(ws), _lib.stream_ptr())
        total += m.numel()
    if counts is None:
        raise _lib.InsarError("label_histogram: no masks")
    host = counts.cpu()
    if int(host.sum()) != total:
        raise _lib.InsarError(f"label_histogram: {total - int(host.sum())} pixels carry a label outside [0, {K}) that is not "
                              f"ignore_index={ignore_index}")
    return (host[:K].clone(), int(host[K])) if return_ignored else host[:K].clone()


def class_weights(counts, scheme: str = "inverse", c: float = 1.02) -> torch.Tensor:
    """Class weights from per-class pixel counts n_c (label_histogram), N = sum n_c, f_c = n_c / N, K = len(counts):
      "inverse": N / (K n_c)            (balanced: a uniform histogram gives ones)
      "median":  median(f) / f_c        (median-frequency balancing; the median is over the classes that occur)
      "enet":    1 / ln(c + f_c)        (ENet, c = 1.02)
    A class without pixels gets weight 0 (it cannot contribute to the loss anyway) and a warning. float32 CPU tensor [K]."""
    n = [float(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    K, N = len(n), sum(n)
    if K < 1 or N <= 0 or any(v < 0 or not math.isfinite(v) for v in n):
        raise _lib.InsarError(f"class_weights: counts must be non-negative with a positive sum, got {n}")
    if scheme not in ("inverse", "median", "enet"):
        raise _lib.InsarError(f"class_weights: scheme={scheme!r} is not one of 'inverse', 'median', 'enet'")
    empty = [i for i, v in enumerate(n) if v == 0]
    if empty:
        warnings.warn(f"class_weights: no pixels of class(es) {empty}; their weight is set to 0", stacklevel=2)
    f = [v / N for v in n]
    present = sorted(v for v in f if v > 0)
    med = present[len(present) // 2] if len(present) % 2 else 0.5 * (present[len(present) // 2 - 1] + present[len(present) // 2])
    if scheme == "inverse":
        w = [N / (K * v) if v > 0 else 0.0 for v in n]
    elif scheme == "median":
        w = [med / v if v > 0 else 0.0 for v in f]
    else:
        w = [1.0 / math.log(c + v) if v > 0 else 0.0 for v in f]
    return torch.tensor(w, dtype=torch.float32)
