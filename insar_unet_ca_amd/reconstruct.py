"""Grey-scale morphological reconstruction on the device (csrc/reconstruct.hip: insar_reconstruct_prepare / _rounds / _finish):
what reads the SHAPE of a continuous raster instead of a class map or a fixed threshold. `fill_sinks` answers "where does this
displacement map have closed depressions, and how deep", `h_dome` "which peaks rise at least h above their surroundings",
`regional_extrema` gives one plateau per peak; `reconstruct_raster` is the operation under all three. `hysteresis_regions` is its
binary special case.

The rule (tests/reconstruct_ref.py restates it twice in numpy; DESIGN.md, "Grey-scale reconstruction"): reconstruction by
dilation of a marker F under a mask G is the pointwise limit of J <- min(G, max of J over the pixel and its 4 or 8 neighbours)
from J = min(F, G); equivalently R(p) is the maximum over all connected paths q -> p of min(F(q), min of G along the path).
Reconstruction by erosion is the order-dual. Only min, max and compare are needed, so everything runs on order-preserving 32-bit
keys of the RAW values (`raster_keys`): nothing is quantised, and every output pixel carries the exact bit pattern of a marker
or mask pixel. The limit is unique, so the result cannot depend on the schedule: it is bitwise reproducible, and so is the
number of rounds.

Invalid pixels are barriers: the `valid` plane, an exact `nodata` compare, a non-finite float32 mask value (a NaN marker value;
a marker of +-inf is taken as it is) and everything outside the raster neither take nor pass a value. Invalid outputs hold NaN
in float32 and `fill` in integer outputs.

2 + rounds launches on the current stream; the host reads the 8-byte counters of ROUNDS_PER_READ rounds at a time and stops at
the first round that changed no tile, or at `max_rounds` (`converged` False: the output then lies between min(F, G) and the
fixed point).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_map, check_on_device, query_bytes, read_back
from .focal import _check_fill, _check_flag, _check_nodata, _check_raster, _is_number, _overlaps
from .hysteresis import from_ordered_u32, ordered_u32

MAX_ROUNDS = _lib.RECONSTRUCT_MAX_ROUNDS
DEFAULT_MAX_ROUNDS = 4096                # the tiles of a 4096 x 4096 scene: a front that crosses one tile per round gets everywhere
ROUNDS_PER_READ = 8                      # the host looks at the counters once per this many rounds

_ELEM = {torch.float32: _lib.ZONAL_F32, torch.uint8: _lib.ZONAL_U8, torch.int32: _lib.ZONAL_I32}
_RESIDUE = {torch.float32: torch.float32, torch.uint8: torch.int32, torch.int32: torch.int32}
_COUNTER_BYTES = 8 * (MAX_ROUNDS + 1)


def reconstruct_tile() -> int:
    """The edge of the square tile one work-group of a round solves. Host arithmetic only."""
    edge = C.c_int32(0)
    call("insar_reconstruct_tile", C.byref(edge))
    return int(edge.value)


def scratch_bytes(H: int, W: int, planes: int = 1) -> int:
    """The bytes of a call's scratch: three key planes, two tile-activity maps and the round counters. Host arithmetic only."""
    return query_bytes("insar_reconstruct_bytes", planes, H, W, outputs=1)


def raster_keys(x) -> np.ndarray:
    """The order-preserving uint32 keys of a float32, int32 or uint8 numpy array: `hysteresis.ordered_u32` (-0.0 directly below
    0.0), the sign bit flipped, the value as it is."""
    x = np.asarray(x)
    if x.dtype == np.float32:
        return ordered_u32(x)
    if x.dtype == np.int32:
        return np.ascontiguousarray(x).view(np.uint32) ^ np.uint32(0x80000000)
    if x.dtype == np.uint8:
        return x.astype(np.uint32)
    raise InsarError(f"raster_keys: {x.dtype} array: float32, int32 or uint8")


def raster_from_keys(k, dtype) -> np.ndarray:
    """The values of `raster_keys` keys in `dtype` (float32, int32 or uint8)."""
    k, dtype = np.ascontiguousarray(k, dtype=np.uint32), np.dtype(dtype)
    if dtype == np.float32:
        return from_ordered_u32(k)
    if dtype == np.int32:
        return (k ^ np.uint32(0x80000000)).view(np.int32)
    if dtype == np.uint8:
        return k.astype(np.uint8)
    raise InsarError(f"raster_from_keys: dtype {dtype}: float32, int32 or uint8")


class ReconstructScratch(Scratch):
    """The device buffers of one (H, W, planes): the two key planes of J, the key plane of G, the tile-activity maps, the round
    counters, and the pinned host words the counters are read back into. Nothing in them has to survive between calls."""
    KEY, SHOW, DEVICE_AT = ("H", "W", "planes"), "{} x {}, planes={}", 3

    def __init__(self, H: int, W: int, planes: int, device: torch.device):
        super().__init__((H, W, planes), device, scratch=scratch_bytes(H, W, planes), host=8 * ROUNDS_PER_READ)


def _check_connectivity(who: str, connectivity) -> int:
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise InsarError(f"{who}: connectivity={connectivity!r}: 4 or 8")
    return int(connectivity)


def _check_out(who: str, name: str, out, shape, dtype, sources):
    """A fresh output (None), or the caller's: of that shape and dtype on the raster's device, sharing no memory with an input."""
    if out is None:
        return None
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != sources[0].device
            or not out.is_contiguous() or any(_overlaps(out, s) for s in sources)):
        raise InsarError(f"{who}: {name} must be a contiguous {dtype} tensor {tuple(shape)} on the raster's device that shares no "
                         f"memory with the marker, the mask or the valid plane")
    return out


def _run(who, marker, raster, mode, flip, connectivity, h, valid, nodata, fill, max_rounds, scratch, out, out_dtype, want):
    """The checks every entry shares (devices last), then prepare, the rounds and finish. `out`: the caller's tensor for the
    entry's main output, of `out_dtype`; `want`: which of "out", "residue", "extrema", "valid" finish writes. Returns (the
    outputs by name, info)."""
    H, W, planes = _check_raster(who, raster, tuple(_ELEM))
    if marker is not None:
        check_map(who, "marker", marker, (raster.dtype,), dims=(raster.dim(),), one_fault=True)
        if tuple(marker.shape) != tuple(raster.shape):
            raise InsarError(f"{who}: marker {tuple(marker.shape)}: expected {tuple(raster.shape)}, the mask's shape")
    if valid is not None:
        check_map(who, "valid", valid, (torch.uint8,), shape=(H, W), of="raster")
    connectivity = _check_connectivity(who, connectivity)
    has_nodata, nd = _check_nodata(who, raster, nodata)
    max_rounds = check_int(who, "max_rounds", max_rounds, 1, MAX_ROUNDS, integral_floats=False)
    sources = [t for t in (raster, marker, valid) if t is not None]
    main = next(n for n in ("out", "residue", "extrema") if n in want)
    out = _check_out(who, "out", out, raster.shape, out_dtype, sources)
    if scratch is not None:
        ReconstructScratch.check(who, scratch, (H, W, planes), raster.device)
    check_on_device(who, "raster" if marker is None else "mask", raster)
    if marker is not None:
        check_on_device(who, "marker", marker, like=raster)
    if valid is not None:
        check_on_device(who, "valid", valid, like=raster)
    dev = raster.device
    if scratch is None:
        scratch = ReconstructScratch(H, W, planes, dev)
    dtypes = {"out": raster.dtype, "residue": _RESIDUE[raster.dtype], "extrema": torch.uint8, "valid": torch.uint8}
    res = {n: torch.empty(raster.shape, dtype=dtypes[n], device=dev) for n in want}
    if out is not None:
        res[main] = out
    buf = scratch.scratch
    counters = buf[buf.numel() - _COUNTER_BYTES:]
    rounds, converged, ran, active = 0, False, 0, 0
    with torch.cuda.device(dev):
        s = _lib.stream_ptr()
        call("insar_reconstruct_prepare", ptr(marker), ptr(raster), _ELEM[raster.dtype], planes, H, W, mode, flip, connectivity, float(h),
             max_rounds, has_nodata, nd, ptr(valid), ptr(buf), s)
        while ran < max_rounds and not converged:
            n = min(ROUNDS_PER_READ, max_rounds - ran)
            call("insar_reconstruct_rounds", planes, H, W, connectivity, ran, n, ptr(buf), s)
            pairs = read_back(scratch.host, counters[8 * ran:8 * (ran + n)], 8 * n).view(np.int32).reshape(n, 2)
            done = np.flatnonzero(pairs[:, 0] == 0)
            converged = done.size > 0
            rounds = ran + (int(done[0]) + 1 if converged else n)
            active += int(pairs[:rounds - ran, 1].sum())
            ran += n
        call("insar_reconstruct_finish", ptr(marker), ptr(raster), _ELEM[raster.dtype], planes, H, W, mode, flip, has_nodata, nd, ptr(valid),
             ran, fill, ptr(buf), ptr(res.get("out")), ptr(res.get("residue")), ptr(res.get("extrema")), ptr(res.get("valid")), s)
    return res, {"rounds": rounds, "converged": converged, "active_tile_rounds": active}


def _answer(parts, info, return_info):
    parts = list(parts) + ([info] if return_info else [])
    return parts[0] if len(parts) == 1 else tuple(parts)


def reconstruct_raster(marker: torch.Tensor, mask: torch.Tensor, *, method: str = "dilation", connectivity: int = 8,
                       valid: Optional[torch.Tensor] = None, nodata: Optional[float] = None, fill: int = 0,
                       max_rounds: int = DEFAULT_MAX_ROUNDS, return_valid: bool = False, return_info: bool = False,
                       scratch: Optional[ReconstructScratch] = None, out: Optional[torch.Tensor] = None):
    """The morphological reconstruction of `marker` under (`method` "dilation") or over ("erosion") `mask`: device rasters [H, W]
    or [C, H, W] of one shape and dtype (float32, uint8 or int32); the result has that dtype.

        rec = reconstruct_raster(seeds, prob)                        # prob where a path from a seed never dips below it
        rec, ok, info = reconstruct_raster(m, g, method="erosion", nodata=-9999.0, return_valid=True, return_info=True)

    A marker above the mask (dilation; below it, erosion) is clamped to it, not refused. `valid`: uint8 [H, W], 0 = barrier;
    `nodata`: an exact compare in the raster's type, on marker and mask. `fill`: what invalid pixels of an integer output hold
    (float32: NaN). `info`: {"rounds": the rounds run up to the first that changed nothing, "converged": False if `max_rounds`
    (1..65535) cut the propagation off, "active_tile_rounds"}. `scratch`: a ReconstructScratch of this shape to reuse; `out`:
    the output tensor, sharing no memory with an input."""
    who = "reconstruct_raster"
    if not isinstance(method, str) or method not in ("dilation", "erosion"):
        raise InsarError(f"{who}: method={method!r}: 'dilation' or 'erosion'")
    return_valid, return_info = _check_flag(who, "return_valid", return_valid), _check_flag(who, "return_info", return_info)
    check_map(who, "mask", mask, tuple(_ELEM), dims=(2, 3), one_fault=True)
    if not isinstance(marker, torch.Tensor):
        raise InsarError(f"{who}: marker must be a torch tensor, got {type(marker).__name__}")
    fill = _check_fill(who, mask, fill)
    res, info = _run(who, marker, mask, _lib.RECONSTRUCT_PLAIN, int(method == "erosion"), connectivity, 0.0, valid, nodata, fill,
                     max_rounds, scratch, out, mask.dtype, ("out", "valid") if return_valid else ("out",))
    return _answer([res["out"]] + ([res["valid"]] if return_valid else []), info, return_info)


def fill_sinks(raster: torch.Tensor, *, invert: bool = False, connectivity: int = 8, valid: Optional[torch.Tensor] = None,
               nodata: Optional[float] = None, fill: int = 0, return_depth: bool = False, max_rounds: int = DEFAULT_MAX_ROUNDS,
               return_valid: bool = False, return_info: bool = False, scratch: Optional[ReconstructScratch] = None,
               out: Optional[torch.Tensor] = None):
    """The raster with every closed depression filled to its spill level: reconstruction by erosion of the marker that equals
    the raster at OUTLETS and the highest key elsewhere. An outlet is a valid pixel on the raster's edge or with a `connectivity`
    neighbour that is invalid; every component of valid pixels has one, so no value is invented.

        filled, depth = fill_sinks(displacement, valid=pred["valid"], return_depth=True)
        bowls = label_regions((depth > 0.02).to(torch.uint8))        # closed depressions at least 2 cm deep

    `invert`: fill domes instead (the other sign convention of line-of-sight displacement). `return_depth` adds filled - raster
    (raster - filled when inverted), never negative: one float32 subtraction, or an exact int32 saturating at 2^31 - 1 for
    integer rasters; NaN / 0 at invalid pixels. A ramp moves the spill level along with the bowl, so it does not change the
    depth. Returns filled [, depth] [, valid] [, info]; the other arguments as `reconstruct_raster`."""
    who = "fill_sinks"
    invert, return_depth = _check_flag(who, "invert", invert), _check_flag(who, "return_depth", return_depth)
    return_valid, return_info = _check_flag(who, "return_valid", return_valid), _check_flag(who, "return_info", return_info)
    check_map(who, "raster", raster, tuple(_ELEM), dims=(2, 3), one_fault=True)
    fill = _check_fill(who, raster, fill)
    want = ("out",) + (("residue",) if return_depth else ()) + (("valid",) if return_valid else ())
    res, info = _run(who, None, raster, _lib.RECONSTRUCT_FILL, int(not invert), connectivity, 0.0, valid, nodata, fill, max_rounds,
                     scratch, out, raster.dtype, want)
    return _answer([res[n] for n in want], info, return_info)


def _check_h(who: str, raster, h) -> float:
    if not _is_number(h) or not math.isfinite(h) or not h > 0:
        raise InsarError(f"{who}: h={h!r}: a positive finite number")
    if raster.dtype == torch.float32:
        with np.errstate(over="ignore"):
            hf = np.float32(h)
        if not (np.isfinite(hf) and hf > 0):
            raise InsarError(f"{who}: h={h!r} is not positive and finite in float32")
        return float(hf)
    if h != int(h) or int(h) > (1 << 31) - 1:
        raise InsarError(f"{who}: h={h!r}: an integer in 1..2^31 - 1 for a {raster.dtype} raster")
    return float(int(h))


def h_dome(raster: torch.Tensor, h, *, invert: bool = False, connectivity: int = 8, valid: Optional[torch.Tensor] = None,
           nodata: Optional[float] = None, max_rounds: int = DEFAULT_MAX_ROUNDS, return_valid: bool = False, return_info: bool = False,
           scratch: Optional[ReconstructScratch] = None, out: Optional[torch.Tensor] = None):
    """The h-domes of a raster: raster - R(raster - h under raster), in 0..h: how far each pixel rises above the level from
    which its peak stands out by `h`. A peak of prominence >= h keeps a dome of height h, a ripple of prominence p < h one of
    height p, so a threshold on the residue tells sites from ripples by prominence.

        domes = h_dome(prob, 0.2)                     # float32; > 0 on every peak, == 0.2 at the top of the prominent ones
        basins = h_dome(displacement, 0.02, invert=True)

    `invert`: the h-basins R - raster by erosion of raster + h. The marker's one operation is float32 (h as float32), or a
    saturating integer one (h an integer) in the prepare kernel; the residue is float32 for a float32 raster, else int32; NaN /
    0 at invalid pixels. Raising h never lowers the residue. Returns residue [, valid] [, info]; `out`: the residue's tensor."""
    who = "h_dome"
    invert = _check_flag(who, "invert", invert)
    return_valid, return_info = _check_flag(who, "return_valid", return_valid), _check_flag(who, "return_info", return_info)
    check_map(who, "raster", raster, tuple(_ELEM), dims=(2, 3), one_fault=True)
    h = _check_h(who, raster, h)
    want = ("residue",) + (("valid",) if return_valid else ())
    res, info = _run(who, None, raster, _lib.RECONSTRUCT_HDOME, int(invert), connectivity, h, valid, nodata, 0, max_rounds, scratch,
                     out, _RESIDUE[raster.dtype], want)
    return _answer([res[n] for n in want], info, return_info)


def regional_extrema(raster: torch.Tensor, kind: str = "max", *, connectivity: int = 8, valid: Optional[torch.Tensor] = None,
                     nodata: Optional[float] = None, max_rounds: int = DEFAULT_MAX_ROUNDS, return_info: bool = False,
                     scratch: Optional[ReconstructScratch] = None, out: Optional[torch.Tensor] = None):
    """uint8 map: 1 on the plateaus (connected sets of equal valid pixels) with no higher (`kind` "max") or lower ("min")
    neighbour, 0 elsewhere and at invalid pixels: one seed per peak, for `hysteresis_regions(min_seeds=)` and peak lists.

        peaks = regional_extrema(prob, "max", valid=pred["valid"])

    In key space the marker is key - 1, saturating at 0, and the output is key > R. A plateau at the order's own end (uint8 0
    or INT32_MIN for "max", INT32_MAX for "min") has the key 0 and nothing to stand above: it is reported as 0. A uint8
    plateau at 255 is a minimum like any other (the complement is taken on the 32-bit key), and float32 has no such value: its
    key 0 is a NaN. Returns the map [, info]."""
    who = "regional_extrema"
    if not isinstance(kind, str) or kind not in ("max", "min"):
        raise InsarError(f"{who}: kind={kind!r}: 'max' or 'min'")
    return_info = _check_flag(who, "return_info", return_info)
    check_map(who, "raster", raster, tuple(_ELEM), dims=(2, 3), one_fault=True)
    res, info = _run(who, None, raster, _lib.RECONSTRUCT_EXTREMA, int(kind == "min"), connectivity, 0.0, valid, nodata, 0, max_rounds,
                     scratch, out, torch.uint8, ("extrema",))
    return _answer([res["extrema"]], info, return_info)


__all__ = ["DEFAULT_MAX_ROUNDS", "ReconstructScratch", "fill_sinks", "h_dome", "raster_from_keys", "raster_keys", "reconstruct_raster",
           "reconstruct_tile", "regional_extrema", "scratch_bytes"]
