"""On-device augmentation (csrc/augment.hip: insar_aug_draw / insar_aug_apply): the eight flips and rotations of the
square (the dihedral group D4) applied to a batch of images and its masks together, a per-sample gain and bias, and additive
noise. The same apply kernel carries the flips and rotations of test-time augmentation (infer.ScenePredictor(tta=...)).

D4 op codes 0..7 on an [H, W] plane `a`, in numpy terms:

    b = a.T if op & 4 else a
    if op & 2: b = b[::-1, :]
    if op & 1: b = b[:, ::-1]

np.rot90(a, 1) is op 6 and np.rot90(a, 3) is op 5; the inverse of an op is itself, except that 5 and 6 invert each other
(`D4_INVERSE`). Everything is a pure function of (seed, rank, step): two runs, or a run resumed from `state_dict()`, see the
same stream of transforms, and nothing is read back from the device per call.
"""
from __future__ import annotations

from typing import Iterable, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr

MASK64 = (1 << 64) - 1
D4_INVERSE = (0, 1, 2, 3, 4, 6, 5, 7)
NOISE_STREAM = 0x5851F42D4C957F2D          # separates the noise seeds from the table's draws
TTA_VALUES = (1, 2, 4, 8)
MAX_SIDE = 32768


def aug_hash64(key: int, i: int) -> int:
    """The hash of csrc/augment.hip on Python integers (uint64 arithmetic with wrap-around)."""
    z = (key + 0x9E3779B97F4A7C15 * (i + 1)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def check_tta(tta) -> int:
    """tta = 1, 2, 4 or 8: the ops 0 .. tta - 1 are averaged (1: none; 2: + horizontal flip; 4: the flips; 8: all of D4)."""
    if isinstance(tta, bool) or not isinstance(tta, (int, np.integer)) or int(tta) not in TTA_VALUES:
        raise InsarError(f"tta={tta!r}: one of {TTA_VALUES} (the ops 0 .. tta - 1 are averaged)")
    return int(tta)


def _ops_mask(ops) -> int:
    if isinstance(ops, str):
        if ops == "d4":
            return 0xff
        if ops == "flips":
            return 0x0f
        raise InsarError(f"ops={ops!r}: 'd4', 'flips' or an iterable of op codes 0..7")
    mask = 0
    try:
        codes = list(ops)
    except TypeError:
        raise InsarError(f"ops={ops!r}: 'd4', 'flips' or an iterable of op codes 0..7") from None
    for op in codes:
        if isinstance(op, bool) or not isinstance(op, (int, np.integer)) or not 0 <= int(op) <= 7:
            raise InsarError(f"ops: {op!r} is not an op code 0..7")
        mask |= 1 << int(op)
    if mask == 0:
        raise InsarError("ops: no op code given")
    return mask


def _range(name: str, r, lowest: Optional[float] = None) -> Tuple[float, float]:
    try:
        lo, hi = (float(v) for v in r)
    except (TypeError, ValueError):
        raise InsarError(f"{name}={r!r}: a (lo, hi) pair of numbers") from None
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        raise InsarError(f"{name}=({lo}, {hi}): needs finite lo <= hi")
    if lowest is not None and lo < lowest:
        raise InsarError(f"{name}=({lo}, {hi}): lo below {lowest}")
    return lo, hi


def _check_batch(images, masks):
    """-> (n, C, H, W, mask dtype code, device) of a batch of which either part may be None."""
    if images is None and masks is None:
        raise InsarError("augment: neither images nor masks")
    ref = images if images is not None else masks
    if not isinstance(ref, torch.Tensor) or not ref.is_cuda:
        raise InsarError("augment: images and masks must be ROCm tensors (no CPU fallback)")
    C = 1
    if images is not None:
        if images.dim() != 4 or images.dtype != torch.float32 or not images.is_contiguous():
            raise InsarError(f"augment: images must be a contiguous float32 [n, C, H, W] tensor, got {images.dtype} {tuple(images.shape)}")
        n, C, H, W = images.shape
    code = _lib.AUG_MASK_NONE
    if masks is not None:
        if not isinstance(masks, torch.Tensor) or masks.device != ref.device:
            raise InsarError("augment: images and masks must lie on one device")
        if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.int64) or not masks.is_contiguous():
            raise InsarError(f"augment: masks must be a contiguous uint8 or int64 [n, H, W] tensor, got {masks.dtype} {tuple(masks.shape)}")
        if images is not None and tuple(masks.shape) != (n, H, W):
            raise InsarError(f"augment: masks {tuple(masks.shape)} do not match images {tuple(images.shape)}")
        n, H, W = masks.shape
        code = _lib.AUG_MASK_U8 if masks.dtype == torch.uint8 else _lib.AUG_MASK_I64
    if n < 1 or C < 1 or H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise InsarError(f"augment: batch of {n} x {C} x {H} x {W} (every extent >= 1, H and W <= {MAX_SIDE})")
    return n, C, H, W, code, ref.device


def apply_table(images: Optional[torch.Tensor], masks: Optional[torch.Tensor], table: torch.Tensor, noise_seed: int = 0,
                out: Optional[tuple] = None):
    """insar_aug_apply on the current stream: row s of `table` (device int32 [n, 4]: op, then the float32 bits of gain,
    bias, sigma) transforms sample s of `images` (float32 [n, C, H, W]) and `masks` (uint8 / int64 [n, H, W]); either may
    be None. Returns (images_out, masks_out) with masks_out int64: fresh tensors, or the pair `out` if given."""
    n, C, H, W, code, dev = _check_batch(images, masks)
    if (not isinstance(table, torch.Tensor) or table.device != dev or table.dtype != torch.int32 or tuple(table.shape) != (n, 4)
            or not table.is_contiguous()):
        raise InsarError(f"augment: the table must be a contiguous int32 [{n}, 4] tensor on {dev}")
    xo, mo = out if out is not None else (None, None)
    if images is not None:
        if xo is None:
            xo = torch.empty_like(images)
        elif xo.shape != images.shape or xo.dtype != torch.float32 or not xo.is_contiguous() or xo.device != dev:
            raise InsarError("augment: out[0] must match the images")
    else:
        xo = None
    if masks is not None:
        if mo is None:
            mo = torch.empty(masks.shape, dtype=torch.int64, device=dev)
        elif mo.shape != masks.shape or mo.dtype != torch.int64 or not mo.is_contiguous() or mo.device != dev:
            raise InsarError("augment: out[1] must be an int64 tensor of the masks' shape")
    else:
        mo = None
    call("insar_aug_apply", ptr(images), ptr(xo), C, ptr(masks), code, ptr(mo), n, H, W, ptr(table), int(noise_seed) & MASK64,
         _lib.stream_ptr())
    return xo, mo


def constant_table(ops: Iterable[int], device) -> torch.Tensor:
    """Device table [len(ops), 4] with row s = {ops[s], gain 1, bias 0, sigma 0}: a pure flip / rotation per sample."""
    ops = list(ops)
    t = np.zeros((len(ops), 4), dtype=np.int32)
    t[:, 0] = np.asarray(ops, dtype=np.int32)
    t[:, 1] = np.float32(1.0).view(np.int32)
    return torch.from_numpy(t).to(device)


class Augment:
    """Random D4 + photometric augmentation of a training batch on the device.

        aug = Augment(seed=0, rank=rank, ops="d4", gain=(0.8, 1.25), bias=(-0.1, 0.1), noise_sigma=(0.0, 0.1))
        images, masks = aug(images, masks)        # fresh device tensors on the current stream; masks come back int64

    Per sample: one op drawn uniformly from `ops` ("d4": all eight, "flips": ops 0..3, or an iterable of op codes) applied
    to the image and its mask alike; x -> gain * x + bias + sigma * z on the image, with gain / bias / sigma uniform in their
    ranges and z approximately unit normal (|z| < 3.47) per element. Call k of an object uses step = k (`aug.step`, which
    the call increments); `rank` separates the streams of data-parallel workers. `state_dict()` / `load_state_dict()` carry
    {seed, rank, step, config}, so that a resumed run continues the same stream. Tiles must be square if a transposing
    op (4..7) is allowed."""

    def __init__(self, seed: int = 0, rank: int = 0, ops: Union[str, Iterable[int]] = "d4", gain=(1.0, 1.0), bias=(0.0, 0.0),
                 noise_sigma=(0.0, 0.0)):
        for name, v in (("seed", seed), ("rank", rank)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise InsarError(f"Augment: {name}={v!r} is not a non-negative integer")
        self.seed, self.rank, self.step = int(seed) & MASK64, int(rank), 0
        self.ops_mask = _ops_mask(ops)
        self.gain, self.bias = _range("gain", gain), _range("bias", bias)
        self.noise_sigma = _range("noise_sigma", noise_sigma, lowest=0.0)

    @property
    def key_seed(self) -> int:
        return aug_hash64(self.seed, self.rank)

    def noise_seed(self, step: int) -> int:
        return aug_hash64(self.key_seed ^ NOISE_STREAM, step)

    def _config(self) -> dict:
        return {"ops_mask": self.ops_mask, "gain": list(self.gain), "bias": list(self.bias), "noise_sigma": list(self.noise_sigma)}

    def state_dict(self) -> dict:
        return {"seed": self.seed, "rank": self.rank, "step": self.step, "config": self._config()}

    def load_state_dict(self, state: dict) -> None:
        try:
            seed, rank, step, cfg = int(state["seed"]), int(state["rank"]), int(state["step"]), state["config"]
            mask = int(cfg["ops_mask"])
            gain, bias = _range("gain", cfg["gain"]), _range("bias", cfg["bias"])
            sigma = _range("noise_sigma", cfg["noise_sigma"], lowest=0.0)
        except (KeyError, TypeError, ValueError) as e:
            raise InsarError(f"Augment.load_state_dict: malformed state ({e!r})") from None
        if seed < 0 or rank < 0 or step < 0 or not 1 <= mask <= 255:
            raise InsarError(f"Augment.load_state_dict: seed={seed}, rank={rank}, step={step}, ops_mask={mask}")
        self.seed, self.rank, self.step = seed & MASK64, rank, step
        self.ops_mask, self.gain, self.bias, self.noise_sigma = mask, gain, bias, sigma

    def draw(self, n: int, device, step: Optional[int] = None) -> torch.Tensor:
        """The table of `n` samples at `step` (default: the current one, which is NOT advanced), filled on the current stream."""
        step = self.step if step is None else int(step)
        # a fresh 16-byte-per-sample buffer per call: the caching allocator hands it out without a synchronisation and
        # keeps calls on different streams from sharing one
        table = torch.empty(int(n), 4, dtype=torch.int32, device=device)
        call("insar_aug_draw", self.key_seed, step & MASK64, int(n), self.ops_mask, self.gain[0], self.gain[1], self.bias[0],
             self.bias[1], self.noise_sigma[0], self.noise_sigma[1], ptr(table), _lib.stream_ptr())
        return table

    def __call__(self, images: Optional[torch.Tensor], masks: Optional[torch.Tensor] = None, out: Optional[tuple] = None):
        n, C, H, W, code, dev = _check_batch(images, masks)
        if (self.ops_mask & 0xf0) and H != W:
            raise InsarError(f"Augment: ops include a transposing op (4..7) but the tiles are {H} x {W}: square tiles, or ops='flips'")
        with torch.cuda.device(dev):
            table = self.draw(n, dev)
            res = apply_table(images, masks, table, self.noise_seed(self.step), out=out)
        self.step += 1
        return res
