"""Neighbourhood operations on a device raster (csrc/focal.hip: insar_focal_smooth / _rank / _gradient): a NaN-aware separable
smoothing in exact integers, min / max / lower-median rank filters and the slope of a float32 raster, with the no-data rules of
every other raster consumer here: a `valid` plane marks no-data, `nodata` is an exact compare in the raster's own type, and a
non-finite float32 is invalid. Outside the raster is invalid too: there is no padding mode, the normalisation by the valid
weight is the border rule. What `.cpu()` plus scipy or a torch convolution with a mask plane would do, without the copy, honouring
the no-data rules and bitwise reproducible (tests/focal_ref.py restates all of it in numpy; DESIGN.md, "Filtering rasters").

One launch per call on the current stream, no atomics, nothing read back and no host-to-device copy: the taps and scalars are
kernel arguments, so a call can sit in a captured graph. Where the centre pixel is invalid the output is invalid unless
`keep_invalid=False` (gap filling, on request). Invalid outputs take NaN in float32 and `fill` in integer outputs;
`return_valid=True` also returns the uint8 plane of valid outputs, which `contour_lines(valid=)` and
`hysteresis_regions(valid=)` take as it is.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import check_int, check_map, check_on_device

MAX_RADIUS = 15
MAX_TAP_SUM = 4096
MAX_MEDIAN_RADIUS = 3
MAX_PLANES = 65535
DEFAULT_SCALE = 2 ** 16

_ELEM = {torch.float32: _lib.ZONAL_F32, torch.uint8: _lib.ZONAL_U8, torch.int32: _lib.ZONAL_I32}
_OPS = {"min": _lib.FOCAL_MIN, "max": _lib.FOCAL_MAX, "median": _lib.FOCAL_MEDIAN}


def focal_tile(radius: int = 0):
    """(rows, columns) of outputs one work-group of the smoothing and min / max kernels computes at `radius`. Host arithmetic
    only."""
    radius = check_int("focal_tile", "radius", radius, 0, MAX_RADIUS, integral_floats=False)
    rows, cols = C.c_int32(0), C.c_int32(0)
    call("insar_focal_tile", radius, C.byref(rows), C.byref(cols))
    return int(rows.value), int(cols.value)


# ---- tap builders (host) ---------------------------------------------------------------------------------------------------
def box_taps(radius: int) -> np.ndarray:
    """2 radius + 1 ones: the mean over the valid pixels of the (2 radius + 1)^2 window."""
    radius = check_int("box_taps", "radius", radius, 0, MAX_RADIUS, integral_floats=False)
    return np.ones(2 * radius + 1, dtype=np.int32)


def gaussian_taps(sigma: float, radius: Optional[int] = None, total: int = 4096) -> np.ndarray:
    """Integer taps of a Gaussian: weights exp(-i^2 / (2 sigma^2)) in float64 over -radius..radius (`radius` defaults to
    ceil(3 sigma)), each side tap floor(w_i / sum(w) * total), the remainder on the centre tap, so that the taps sum to `total`
    exactly. One side is computed and mirrored: the taps are symmetric."""
    who = "gaussian_taps"
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not math.isfinite(sigma) or sigma <= 0:
        raise InsarError(f"{who}: sigma={sigma!r}: a positive finite number")
    if radius is None:
        radius = int(math.ceil(3.0 * float(sigma)))
        if radius > MAX_RADIUS:
            raise InsarError(f"{who}: sigma={sigma!r}: radius ceil(3 sigma) = {radius} exceeds {MAX_RADIUS}; give a radius")
    radius = check_int(who, "radius", radius, 0, MAX_RADIUS, integral_floats=False)
    total = check_int(who, "total", total, 1, MAX_TAP_SUM, integral_floats=False)
    i = np.arange(0, radius + 1, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * float(sigma) * float(sigma)))
    norm = w[0] + 2.0 * w[1:].sum()
    side = np.floor(w[1:] / norm * total).astype(np.int64)
    centre = total - 2 * int(side.sum())
    return np.concatenate([side[::-1], [centre], side]).astype(np.int32)


def check_taps(who: str, taps) -> np.ndarray:
    """int32 [2 R + 1] from a sequence of non-negative integers: 0 <= R <= 15, 1 <= sum <= 4096; else InsarError."""
    if isinstance(taps, torch.Tensor) or isinstance(taps, (str, bytes)):
        raise InsarError(f"{who}: taps must be a host sequence of 2 R + 1 non-negative integers, got {type(taps).__name__}")
    try:
        arr = np.asarray(taps)
    except Exception:
        raise InsarError(f"{who}: taps={taps!r}: a sequence of 2 R + 1 non-negative integers") from None
    if arr.ndim != 1 or arr.size % 2 != 1 or arr.size > 2 * MAX_RADIUS + 1 or arr.dtype.kind not in "iu":
        raise InsarError(f"{who}: taps: a 1-D sequence of 2 R + 1 integers, 0 <= R <= {MAX_RADIUS}, got shape {arr.shape} of {arr.dtype}")
    if (arr < 0).any():
        raise InsarError(f"{who}: taps hold a negative entry: every tap is >= 0")
    total = sum(int(v) for v in arr)
    if not 1 <= total <= MAX_TAP_SUM:
        raise InsarError(f"{who}: taps sum to {total}: 1 <= sum <= {MAX_TAP_SUM}")
    return arr.astype(np.int32)


def coverage_threshold(min_coverage: float, tap_sum: int) -> int:
    """T = max(1, ceil(min_coverage * S^2)) in float64: an output is valid iff its valid weight D >= T."""
    return max(1, int(math.ceil(float(min_coverage) * float(tap_sum * tap_sum))))


# ---- the argument checks the three operations share ---------------------------------------------------------------------------
def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _check_raster(who: str, raster, dtypes):
    check_map(who, "raster", raster, dtypes, dims=(2, 3), one_fault=True)
    H, W = (int(v) for v in raster.shape[-2:])
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise InsarError(f"{who}: raster {H} x {W}: need H, W >= 1 and H * W < 2^31")
    planes = 1 if raster.dim() == 2 else int(raster.shape[0])
    if not 1 <= planes <= MAX_PLANES:
        raise InsarError(f"{who}: raster {tuple(raster.shape)}: 1..{MAX_PLANES} planes")
    return H, W, planes


def _check_nodata(who: str, raster, nodata):
    """(has_nodata, nodata as a float): the rule of `region_stats`."""
    if nodata is None:
        return 0, 0.0
    if not _is_number(nodata):
        raise InsarError(f"{who}: nodata={nodata!r}: a number or None")
    nd = float(nodata)
    if math.isnan(nd):
        raise InsarError(f"{who}: nodata is NaN: NaN pixels are invalid already, and nothing equals NaN")
    if raster.dtype != torch.float32:
        lo, hi = (0, 255) if raster.dtype == torch.uint8 else (-(1 << 31), (1 << 31) - 1)
        if nd != int(nd) or not lo <= int(nd) <= hi:
            raise InsarError(f"{who}: nodata={nodata!r} is no value of a {raster.dtype} raster")
    return 1, nd


def _check_fill(who: str, raster, fill) -> int:
    if raster.dtype == torch.float32:
        if not _is_number(fill) or fill != 0:
            raise InsarError(f"{who}: fill={fill!r}: invalid float32 outputs are NaN; fill is for integer outputs")
        return 0
    lo, hi = (0, 255) if raster.dtype == torch.uint8 else (-(1 << 31), (1 << 31) - 1)
    return check_int(who, "fill", fill, lo, hi, integral_floats=False, expect=f"a value of a {raster.dtype} raster")


def _check_flag(who: str, name: str, v) -> bool:
    if not isinstance(v, (bool, np.bool_)):
        raise InsarError(f"{who}: {name}={v!r}: True or False")
    return bool(v)


def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _check_out(who: str, raster, out, shape, dtype):
    """A fresh output, or the caller's: checked like `warp_raster(out=)`; a neighbourhood is read after its centre is written,
    so `out` may not share memory with the raster."""
    if out is None:
        return None
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != raster.device
            or not out.is_contiguous() or _overlaps(out, raster)):
        raise InsarError(f"{who}: out must be a contiguous {dtype} tensor {tuple(shape)} on the raster's device that shares no "
                         f"memory with the raster")
    return out


def _check_common(who, raster, dtypes, valid, nodata, keep_invalid, return_valid):
    H, W, planes = _check_raster(who, raster, dtypes)
    if valid is not None:
        check_map(who, "valid", valid, (torch.uint8,), shape=(H, W), of="raster")
    has_nodata, nd = _check_nodata(who, raster, nodata)
    return H, W, planes, has_nodata, nd, _check_flag(who, "keep_invalid", keep_invalid), _check_flag(who, "return_valid", return_valid)


def _check_devices(who, raster, valid):
    check_on_device(who, "raster", raster)
    if valid is not None:
        check_on_device(who, "valid", valid, like=raster)


# ---- 1. smoothing ----------------------------------------------------------------------------------------------------------------
def smooth_raster(raster: torch.Tensor, taps: Sequence[int], *, scale: float = DEFAULT_SCALE, valid: Optional[torch.Tensor] = None,
                  nodata: Optional[float] = None, min_coverage: float = 0.0, keep_invalid: bool = True, fill: int = 0,
                  return_valid: bool = False, out: Optional[torch.Tensor] = None):
    """A separable normalised convolution of a device raster [H, W] or [C, H, W] (float32, uint8 or int32) in exact integers:
    the weighted mean of the VALID pixels under `taps` x `taps`.

        smooth = smooth_raster(height, gaussian_taps(1.5), valid=pred["valid"])
        smooth, ok = smooth_raster(coherence, box_taps(2), nodata=-9999.0, min_coverage=0.5, return_valid=True)

    `taps`: `box_taps(R)`, `gaussian_taps(sigma)` or 2 R + 1 non-negative integers of your own (0 <= R <= 15, 1 <= sum S <=
    4096; tap i multiplies the pixel at offset i - R: correlation, nothing is flipped; the same taps serve rows and columns).
    A float32 pixel becomes q = rint(clamp(float64(v) * scale, +-(2^31 - 1))), ties to even (`zonal`'s rule); integer rasters
    are taken as they are and refuse a `scale`. With N the tap-weighted sum of the valid q and D the tap weight of the valid
    pixels, the output is valid iff D >= max(1, ceil(min_coverage * S^2)) (`min_coverage` in 0..1) and holds
    floor((2 N + D) / (2 D)): round to nearest, ties towards +infinity for both signs; float32 outputs are that integer over
    `scale`. A constant raster comes back as its own quantisation under any validity pattern. Returns the smoothed raster (the
    input's dtype and shape), with `return_valid` also the uint8 plane of valid outputs."""
    who = "smooth_raster"
    H, W, planes, has_nodata, nd, keep_invalid, return_valid = _check_common(who, raster, tuple(_ELEM), valid, nodata, keep_invalid,
                                                                             return_valid)
    k = check_taps(who, taps)
    if not _is_number(scale) or not math.isfinite(scale) or scale <= 0:
        raise InsarError(f"{who}: scale={scale!r}: a positive finite number")
    if raster.dtype != torch.float32 and scale != DEFAULT_SCALE:
        raise InsarError(f"{who}: scale={scale!r}: a {raster.dtype} raster is taken as it is; scale is for float32")
    if not _is_number(min_coverage) or not 0.0 <= min_coverage <= 1.0:
        raise InsarError(f"{who}: min_coverage={min_coverage!r}: a number in 0..1")
    threshold = coverage_threshold(min_coverage, int(k.sum()))
    fill = _check_fill(who, raster, fill)
    out = _check_out(who, raster, out, raster.shape, raster.dtype)
    _check_devices(who, raster, valid)
    if out is None:
        out = torch.empty_like(raster)
    ok = torch.empty(raster.shape, dtype=torch.uint8, device=raster.device) if return_valid else None
    host_taps = (C.c_int32 * len(k))(*k.tolist())
    with torch.cuda.device(raster.device):
        call("insar_focal_smooth", ptr(raster), _ELEM[raster.dtype], planes, H, W, host_taps, len(k) // 2, float(scale), has_nodata, nd,
             ptr(valid), threshold, int(keep_invalid), fill, ptr(out), ptr(ok), _lib.stream_ptr())
    return (out, ok) if return_valid else out


# ---- 2. rank filters ---------------------------------------------------------------------------------------------------------------
def rank_filter(raster: torch.Tensor, op: str, radius: int, *, valid: Optional[torch.Tensor] = None, nodata: Optional[float] = None,
                min_count: int = 1, keep_invalid: bool = True, fill: int = 0, return_valid: bool = False,
                out: Optional[torch.Tensor] = None):
    """`op` = "min", "max" or "median" over the n valid pixels of the (2 radius + 1)^2 window of a device raster [H, W] or
    [C, H, W] (float32, uint8 or int32), on the raw values: no value appears that was not in the input. float32 values are
    ordered by `hysteresis.ordered_u32` (-0.0 directly below 0.0) and the output is the exact bit pattern of the chosen pixel.
    "min" / "max": 1 <= radius <= 15. "median": 1 <= radius <= 3, the LOWER median, element (n - 1) // 2 of the sorted valid
    values; nothing is averaged. The output is valid iff n >= `min_count`. Returns the filtered raster, with `return_valid`
    also the uint8 plane of valid outputs."""
    who = "rank_filter"
    H, W, planes, has_nodata, nd, keep_invalid, return_valid = _check_common(who, raster, tuple(_ELEM), valid, nodata, keep_invalid,
                                                                             return_valid)
    if not isinstance(op, str) or op not in _OPS:
        raise InsarError(f"{who}: op={op!r}: 'min', 'max' or 'median'")
    radius = check_int(who, "radius", radius, 1, MAX_MEDIAN_RADIUS if op == "median" else MAX_RADIUS, integral_floats=False)
    min_count = check_int(who, "min_count", min_count, 1, (2 * radius + 1) ** 2, integral_floats=False)
    fill = _check_fill(who, raster, fill)
    out = _check_out(who, raster, out, raster.shape, raster.dtype)
    _check_devices(who, raster, valid)
    if out is None:
        out = torch.empty_like(raster)
    ok = torch.empty(raster.shape, dtype=torch.uint8, device=raster.device) if return_valid else None
    with torch.cuda.device(raster.device):
        call("insar_focal_rank", ptr(raster), _ELEM[raster.dtype], planes, H, W, _OPS[op], radius, has_nodata, nd, ptr(valid), min_count,
             int(keep_invalid), fill, ptr(out), ptr(ok), _lib.stream_ptr())
    return (out, ok) if return_valid else out


# ---- 3. slope ------------------------------------------------------------------------------------------------------------------------
def reciprocal_spacing(who: str, spacing):
    """(hy1, hy2, hx1, hx2) as float32: h1 = float32(1 / d), h2 = float32(1 / (2 d)) of spacing = (dy, dx); each positive and
    finite in float32, else InsarError."""
    try:
        dy, dx = spacing
        ok = all(_is_number(d) and math.isfinite(d) and d > 0 for d in (dy, dx))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise InsarError(f"{who}: spacing={spacing!r}: (dy, dx), positive finite numbers")
    with np.errstate(over="ignore"):
        h = [np.float32(1.0 / float(d) / f) for d in (dy, dx) for f in (1.0, 2.0)]
    if not all(np.isfinite(v) and v > 0 for v in h):
        raise InsarError(f"{who}: spacing={spacing!r}: 1 / spacing leaves the float32 range")
    return tuple(h)


def gradient_raster(raster: torch.Tensor, *, spacing=(1.0, 1.0), valid: Optional[torch.Tensor] = None, nodata: Optional[float] = None,
                    keep_invalid: bool = True, return_valid: bool = False, out: Optional[torch.Tensor] = None):
    """The slope of a float32 device raster [H, W] or [C, H, W]: float32 [2, H, W] or [C, 2, H, W] holding gy then gx, in a
    fixed order of float32 operations (no fused multiply-add). Along x, with h1 = float32(1 / dx), h2 = float32(1 / (2 dx)):
    both neighbours valid (v[x+1] - v[x-1]) * h2; only the centre and x + 1 valid (v[x+1] - v[x]) * h1; only the centre and
    x - 1 valid (v[x] - v[x-1]) * h1; otherwise NaN. y likewise with `spacing` = (dy, dx). A component is valid on its own
    terms; the plane of `return_valid` marks the pixels where both are. There is no magnitude plane: combine the two with torch."""
    who = "gradient_raster"
    H, W, planes, has_nodata, nd, keep_invalid, return_valid = _check_common(who, raster, (torch.float32,), valid, nodata, keep_invalid,
                                                                             return_valid)
    hy1, hy2, hx1, hx2 = reciprocal_spacing(who, spacing)
    shape = (2, H, W) if raster.dim() == 2 else (planes, 2, H, W)
    out = _check_out(who, raster, out, shape, torch.float32)
    _check_devices(who, raster, valid)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=raster.device)
    ok = torch.empty(raster.shape, dtype=torch.uint8, device=raster.device) if return_valid else None
    with torch.cuda.device(raster.device):
        call("insar_focal_gradient", ptr(raster), planes, H, W, float(hy1), float(hy2), float(hx1), float(hx2), has_nodata, nd, ptr(valid),
             int(keep_invalid), ptr(out), ptr(ok), _lib.stream_ptr())
    return (out, ok) if return_valid else out


__all__ = ["box_taps", "check_taps", "coverage_threshold", "focal_tile", "gaussian_taps", "gradient_raster", "rank_filter",
           "reciprocal_spacing", "smooth_raster"]
