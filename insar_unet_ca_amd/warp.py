"""Resampling rasters on the device (csrc/warp.hip): a fixed-point affine warp for rasters and label maps, the exact box mean
(multilook), and random rotation / zoom for the crops of `SceneCrops`.

A warp is a 2 x 3 matrix from destination pixel indices (x, y) to source pixel indices, an integer index being a pixel
centre: sx = a x + b y + c, sy = d x + e y + f. It is quantised once on the host to six int64 in Q32 (`quantise_matrix`);
from there on everything that decides anything is integer (include/insar_hip.h states the arithmetic, tests/warp_ref.py
restates it in numpy): positions are cut to 1/256 pixel, a destination pixel is inside iff its centre lies on the source's
pixel extent, everything else is `fill`. `nearest` serves every dtype and is the only mode for label maps; `bilinear` is
integer arithmetic on uint8 and a fixed order of float32 operations on float32, where a NaN tap gives NaN.

    m = grid_matrix(coherence_transform, scene_transform)           # two pixel -> world affines, as to_polygons takes them
    coh = warp_raster(coherence, m, scene.shape)                     # now co-registered: region_stats(labels, coh)
    small = multilook(scene, 4)                                      # predict on it, then bring the mask back:
    mask = warp_raster(small_mask, [[0.25, 0, -0.375], [0, 0.25, -0.375]], scene.shape, mode="nearest", fill=255)

The random warps of a batch are a pure function of the batch key (`draw_warps`: insar_warp_draw), written on the device
from the origins that `draw_crops` drew; nothing is read back."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import check_int, check_on_device, inverse_affine, is_int
from .augment import MASK64

WARP_STREAM = 0x9FB21C651E98DF25            # separates the warp draws from the crop draws of one batch key
Q32 = 1 << 32
ANGLES = 1024                                # the angle table covers the circle in 1024 steps
MAX_ENTRY = float(1 << 20)                   # |matrix entry| <= 2^20 pixels
MAX_DIM = 32768                              # output height and width
MAX_CHANNELS = 4
MAX_ZOOM_Q8 = 4096                           # 16 source pixels per output pixel
_MODES = {"nearest": _lib.WARP_NEAREST, "bilinear": _lib.WARP_BILINEAR}
_DTYPES = {torch.uint8: _lib.WARP_U8, torch.int32: _lib.WARP_I32, torch.float32: _lib.WARP_F32}
_MASK_CODES = {torch.uint8: _lib.AUG_MASK_U8, torch.int64: _lib.AUG_MASK_I64}
_ANGLE_TABLES = {}


def quantise_matrix(matrix) -> np.ndarray:
    """int64 [6] = rint(matrix * 2^32) of a float 2 x 3 destination -> source matrix, in float64 (exact: |entry| <= 2^20)."""
    try:
        m = np.asarray(matrix, dtype=np.float64)
    except (TypeError, ValueError):
        raise InsarError(f"matrix {matrix!r}: a float 2 x 3 array") from None
    if m.shape != (2, 3):
        raise InsarError(f"matrix must be 2 x 3 (destination -> source pixel indices), got shape {m.shape}")
    if not np.isfinite(m).all():
        raise InsarError("matrix has entries that are not finite")
    if (np.abs(m) > MAX_ENTRY).any():
        raise InsarError(f"matrix has entries beyond +-2^20: {m.tolist()}")
    return np.rint(m * float(Q32)).astype(np.int64).reshape(6)


def check_extent(q: np.ndarray, h: int, w: int) -> None:
    """Refuse a Q32 matrix whose positions over an h x w output could leave int64 (host integers)."""
    a, b, c, d, e, f = (int(v) for v in q)
    for p, r, s in ((a, b, c), (d, e, f)):
        if abs(p) * (w - 1) + abs(r) * (h - 1) + abs(s) + (1 << 23) >= 1 << 63:
            raise InsarError(f"matrix over a {h} x {w} output leaves the Q32 range of int64")


def angle_table() -> np.ndarray:
    """int32 [1024, 2]: entry j = (rint(cos(2 pi j / 1024) 2^30), rint(sin(2 pi j / 1024) 2^30)), float64 on the host. The
    quarter turns are exact: (2^30, 0), (0, 2^30), (-2^30, 0), (0, -2^30)."""
    t = 2.0 * np.pi * np.arange(ANGLES, dtype=np.float64) / ANGLES
    return np.stack([np.rint(np.cos(t) * (1 << 30)), np.rint(np.sin(t) * (1 << 30))], axis=1).astype(np.int32)


def _device_angles(device: torch.device) -> torch.Tensor:
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _ANGLE_TABLES:
        _ANGLE_TABLES[key] = torch.from_numpy(angle_table()).to(device)
    return _ANGLE_TABLES[key]


def grid_matrix(src_transform, dst_transform) -> np.ndarray:
    """float64 [2, 3]: the destination -> source matrix in pixel indices of two rasters whose 2 x 3 affines take the lattice
    (x, y) to world coordinates, world = A @ (x, y, 1), in the convention of `to_polygons(transform=)` and `from_geojson`:
    lattice points are pixel corners, pixel (i, j) has its centre at lattice (j + 0.5, i + 0.5). The source transform is
    inverted as `pack_polygons` inverts one; a singular or non-finite transform raises InsarError."""
    inv, t = inverse_affine(src_transform)
    B = np.asarray(dst_transform, dtype=np.float64)
    if B.shape != (2, 3):
        raise InsarError(f"transform must be a 2 x 3 affine, got shape {B.shape}")
    if not np.isfinite(B).all() or B[0, 0] * B[1, 1] - B[0, 1] * B[1, 0] == 0:
        raise InsarError("transform is singular or not finite")
    lin = inv @ B[:, :2]
    off = inv @ (B[:, 2] + B[:, :2] @ np.array([0.5, 0.5]) - t) - 0.5
    return np.concatenate([lin, off[:, None]], axis=1)


def _check_source(who: str, src, dtypes) -> Tuple[int, int, int]:
    check_on_device(who, "src", src)
    if src.dtype not in dtypes:
        raise InsarError(f"{who}: src dtype {src.dtype}: {' or '.join(str(d) for d in dtypes)}")
    if src.dim() not in (2, 3) or not src.is_contiguous():
        raise InsarError(f"{who}: src must be a contiguous [H, W] or planar [C, H, W] tensor, got {tuple(src.shape)}")
    C = 1 if src.dim() == 2 else int(src.shape[0])
    H, W = int(src.shape[-2]), int(src.shape[-1])
    if not 1 <= C <= MAX_CHANNELS:
        raise InsarError(f"{who}: {C} channels: 1..{MAX_CHANNELS}")
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise InsarError(f"{who}: source {H} x {W}: at least one pixel and fewer than 2^31")
    return C, H, W


def _fill_bits(fill, dtype: torch.dtype) -> int:
    if fill is None:
        fill = float("nan") if dtype == torch.float32 else 0
    if isinstance(fill, bool) or not isinstance(fill, (int, float, np.integer, np.floating)):
        raise InsarError(f"fill={fill!r}: a number")
    if dtype == torch.float32:
        return int(np.array([fill], dtype=np.float32).view(np.uint32)[0])
    lo, hi = (0, 255) if dtype == torch.uint8 else (-(1 << 31), (1 << 31) - 1)
    if float(fill) != int(fill) or not lo <= int(fill) <= hi:
        raise InsarError(f"fill={fill!r}: an integer in {lo}..{hi} for {dtype}")
    return int(fill) & 0xFFFFFFFF


def _check_matrices(who: str, matrices, device: torch.device) -> int:
    if (not isinstance(matrices, torch.Tensor) or matrices.device != device or matrices.dtype != torch.int64 or matrices.dim() != 2
            or matrices.shape[1] != 6 or matrices.shape[0] < 1 or not matrices.is_contiguous()):
        raise InsarError(f"{who}: a table of warps must be a contiguous int64 [n, 6] tensor (Q32) on the source's device")
    return int(matrices.shape[0])


def warp_raster(src: torch.Tensor, matrix, out_shape: Sequence[int], *, mode: str = "bilinear", fill=None,
                return_valid: bool = False, out: Optional[torch.Tensor] = None):
    """Resample a device raster onto another pixel grid (insar_warp_raster, 1 launch on the current stream).

    `src`: uint8, int32 or float32, [H, W] or planar [C, H, W] with C <= 4. `matrix`: a float 2 x 3 destination -> source
    matrix in pixel-centre indices (`grid_matrix` builds one from two georeferences), quantised here to Q32; or a device
    table int64 [n, 6] of Q32 warps (`draw_warps`), which gives n outputs. `out_shape` = (h, w). `mode`: "bilinear" or
    "nearest" (int32 and label maps: nearest only). `fill`: the value of pixels whose centre lies off the source; NaN for
    float32 and 0 otherwise by default. Returns a tensor of src's dtype shaped like src with (h, w) in place of (H, W), behind
    a leading n for a table; with `return_valid` also the uint8 plane(s) [h, w] / [n, h, w] that mark the inside pixels."""
    who = "warp_raster"
    C, H, W = _check_source(who, src, tuple(_DTYPES))
    if mode not in _MODES:
        raise InsarError(f"{who}: mode {mode!r}: 'bilinear' or 'nearest'")
    if mode == "bilinear" and src.dtype == torch.int32:
        raise InsarError(f"{who}: bilinear on int32 is refused (label maps take mode='nearest')")
    try:
        h, w = (int(v) for v in out_shape)
    except (TypeError, ValueError):
        raise InsarError(f"{who}: out_shape {out_shape!r}: (h, w)") from None
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        raise InsarError(f"{who}: out_shape {h} x {w}: each of 1..{MAX_DIM}")
    bits = _fill_bits(fill, src.dtype)
    table = isinstance(matrix, torch.Tensor) and matrix.dtype == torch.int64
    if table:
        n = _check_matrices(who, matrix, src.device)
        mats = matrix
    else:
        if isinstance(matrix, torch.Tensor):
            matrix = matrix.detach().cpu().numpy()
        q = quantise_matrix(matrix)
        check_extent(q, h, w)
        n = 1
    shape = ((n,) if table else ()) + tuple(src.shape[:-2]) + (h, w)
    if out is None:
        out = torch.empty(shape, dtype=src.dtype, device=src.device)
    elif (not isinstance(out, torch.Tensor) or out.shape != shape or out.dtype != src.dtype or out.device != src.device
          or not out.is_contiguous() or out.data_ptr() == src.data_ptr()):
        raise InsarError(f"{who}: out must be a contiguous {src.dtype} tensor {shape} on the source's device, not src itself")
    with torch.cuda.device(src.device):
        if not table:
            mats = torch.from_numpy(q.reshape(1, 6)).to(src.device)
        valid = torch.empty(((n,) if table else ()) + (h, w), dtype=torch.uint8, device=src.device) if return_valid else None
        call("insar_warp_raster", ptr(src), _DTYPES[src.dtype], C, H, W, ptr(mats), n, h, w, _MODES[mode], bits, ptr(out), ptr(valid),
             _lib.stream_ptr())
    return (out, valid) if return_valid else out


def multilook(src: torch.Tensor, fy: int, fx: Optional[int] = None, *, min_valid: int = 1, return_count: bool = False):
    """The exact box mean over fy x fx pixels (insar_multilook, 1 launch): [H, W] or [C, H, W] -> [.., H // fy, W // fx], the
    remainder rows and columns dropped; factors 1..16, fx = fy by default. uint8: (sum + n // 2) // n. float32: the mean of
    the values that are not NaN, summed in float32 row by row and left to right, NaN where fewer than `min_valid` are valid.
    `return_count` adds the int32 plane of valid counts. Label maps are not averaged: use warp_raster(mode="nearest")."""
    who = "multilook"
    C, H, W = _check_source(who, src, (torch.uint8, torch.float32))
    fx = fy if fx is None else fx
    for name, v in (("fy", fy), ("fx", fx), ("min_valid", min_valid)):
        if not is_int(v):
            raise InsarError(f"{who}: {name}={v!r}: an integer")
    fy, fx, min_valid = int(fy), int(fx), int(min_valid)
    if not (1 <= fy <= 16 and 1 <= fx <= 16):
        raise InsarError(f"{who}: factors {fy} x {fx}: each of 1..16")
    if fy > H or fx > W:
        raise InsarError(f"{who}: factors {fy} x {fx} above the source {H} x {W}")
    if not 1 <= min_valid <= fy * fx:
        raise InsarError(f"{who}: min_valid={min_valid}: 1..{fy * fx}")
    shape = tuple(src.shape[:-2]) + (H // fy, W // fx)
    with torch.cuda.device(src.device):
        out = torch.empty(shape, dtype=src.dtype, device=src.device)
        count = torch.empty(shape, dtype=torch.int32, device=src.device) if return_count else None
        call("insar_multilook", ptr(src), _DTYPES[src.dtype], C, H, W, fy, fx, min_valid, ptr(out), ptr(count), _lib.stream_ptr())
    return (out, count) if return_count else out


class WarpSpec:
    """The random rotation and zoom of `SceneCrops(warp=...)` and `draw_warps`: `zoom` = (lo, hi) in source pixels per
    output pixel (above 1 the crop sees more of the scene), drawn in steps of 1/256; `max_angle_deg` in 0..180, the rotation
    is drawn in steps of 360 / 1024 degrees from [-max, +max]. WarpSpec() is the identity."""

    def __init__(self, zoom: Tuple[float, float] = (1.0, 1.0), max_angle_deg: float = 0.0):
        try:
            lo, hi = (float(v) for v in zoom)
            ang = float(max_angle_deg)
        except (TypeError, ValueError):
            raise InsarError(f"WarpSpec: zoom={zoom!r}, max_angle_deg={max_angle_deg!r}: (lo, hi) and a number") from None
        if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi):
            raise InsarError(f"WarpSpec: zoom={zoom!r}: 0 < lo <= hi")
        self.zoom_lo, self.zoom_hi = int(np.rint(lo * 256)), int(np.rint(hi * 256))
        if not 1 <= self.zoom_lo <= self.zoom_hi <= MAX_ZOOM_Q8:
            raise InsarError(f"WarpSpec: zoom={zoom!r}: between 1/256 and {MAX_ZOOM_Q8 // 256}")
        if not (np.isfinite(ang) and 0.0 <= ang <= 180.0):
            raise InsarError(f"WarpSpec: max_angle_deg={max_angle_deg!r}: 0..180")
        self.amax = int(np.rint(ang * ANGLES / 360.0))

    def config(self) -> dict:
        return {"zoom_q8": [self.zoom_lo, self.zoom_hi], "amax": self.amax}

    def __repr__(self) -> str:
        return f"WarpSpec(zoom=({self.zoom_lo / 256}, {self.zoom_hi / 256}), max_angle_deg={self.amax * 360.0 / ANGLES})"


def draw_warps(key: int, origins: torch.Tensor, tile: int, spec: WarpSpec) -> torch.Tensor:
    """insar_warp_draw on the current stream -> int64 [n, 6] on the device: one Q32 warp per row of the device table
    `origins` (int32 [n, 2], as `draw_crops` returns it), a rotation and zoom about the centre of its tile x tile crop, a pure
    function of (key, row). WarpSpec() gives the warps under which `gather_warped` equals `gather_crops`."""
    if not isinstance(spec, WarpSpec):
        raise InsarError("draw_warps: spec must be a WarpSpec")
    if (not isinstance(origins, torch.Tensor) or not origins.is_cuda or origins.dtype != torch.int32 or origins.dim() != 2
            or origins.shape[1] != 2 or origins.shape[0] < 1 or not origins.is_contiguous()):
        raise InsarError("draw_warps: origins must be a contiguous int32 [n, 2] ROCm tensor")
    check_int("draw_warps", "tile", tile, 1, MAX_DIM, integral_floats=False)
    n = int(origins.shape[0])
    with torch.cuda.device(origins.device):
        angles = _device_angles(origins.device)
        mats = torch.empty(n, 6, dtype=torch.int64, device=origins.device)
        call("insar_warp_draw", int(key) & MASK64, ptr(origins), n, int(tile), spec.amax, spec.zoom_lo, spec.zoom_hi, ptr(angles),
             ptr(mats), _lib.stream_ptr())
    return mats


def gather_warped(scene: Optional[torch.Tensor], labels: Optional[torch.Tensor], matrices: torch.Tensor, tile: int,
                  mask_dtype: torch.dtype = torch.int64, fill: float = 0.0):
    """insar_warp_gather on the current stream: `gather_crops` through a table of warps -> (images float32 [n, 1, tile, tile]
    or None, masks [n, tile, tile] or None). Images are interpolated bilinearly (a uint8 scene is then normalised like
    `data.reference_transforms`), labels are taken from the nearest pixel; where a crop leaves the scene the image is `fill`
    and the label 255 (void)."""
    who = "gather_warped"
    ref = scene if scene is not None else labels
    if ref is None:
        raise InsarError(f"{who}: neither a scene nor labels")
    for name, t, dts in (("scene", scene, (torch.uint8, torch.float32)), ("labels", labels, (torch.uint8,))):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or t.dtype not in dts or not t.is_contiguous():
            raise InsarError(f"{who}: {name} must be a contiguous 2-D ROCm tensor of dtype {' or '.join(str(d) for d in dts)}")
        if t.shape != ref.shape or t.device != ref.device:
            raise InsarError(f"{who}: scene and labels must have one shape and lie on one device")
    if mask_dtype not in _MASK_CODES:
        raise InsarError(f"{who}: mask_dtype {mask_dtype}: torch.int64 or torch.uint8")
    n = _check_matrices(who, matrices, ref.device)
    if check_int(who, "tile", tile, 4, MAX_DIM, integral_floats=False) % 4:
        raise InsarError(f"{who}: tile={tile!r}: a positive multiple of 4, at most {MAX_DIM}")
    if isinstance(fill, bool) or not isinstance(fill, (int, float, np.integer, np.floating)):
        raise InsarError(f"{who}: fill={fill!r}: a number")
    H, W = (int(v) for v in ref.shape)
    if H * W >= 1 << 31:
        raise InsarError(f"{who}: scene {H} x {W}: fewer than 2^31 pixels")
    tile = int(tile)
    with torch.cuda.device(ref.device):
        images = torch.empty(n, 1, tile, tile, dtype=torch.float32, device=ref.device) if scene is not None else None
        masks = torch.empty(n, tile, tile, dtype=mask_dtype, device=ref.device) if labels is not None else None
        code = _lib.SCENE_F32 if scene is not None and scene.dtype == torch.float32 else _lib.SCENE_U8
        call("insar_warp_gather", ptr(scene), code, ptr(labels), H, W, ptr(matrices), n, tile, float(fill), ptr(images), ptr(masks),
             _MASK_CODES[mask_dtype], _lib.stream_ptr())
    return images, masks
