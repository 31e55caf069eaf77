"""Whole-scene inference: cut a scene into overlapping tiles, run the eval-mode forward of any net of this package on
them, and stitch the class probabilities back together on the device (csrc/scene.hip: insar_scene_gather / _blend /
_finalize). The reference stops at fixed-size tiles; this is what its nets are trained for.

Tiling rule (`plan_tiles`): along each axis origins 0, s, 2s, ... with s = tile - overlap while origin + tile <= size, then
one more tile flush with the edge if the last one is not. Every tile lies inside the scene: there is no padding path, and a
scene smaller than a tile is refused. Window (`window_1d`): the separable trapezoid r(i) = min(i + 1, tile - i, o + 1) / (o + 1).

The stitch is bitwise reproducible and independent of the batch size: a pixel's contributions are added in ascending tile
index (row-major over the tile grid) by the thread that owns the pixel; no atomics. The nets' own forward is NOT promised
bitwise equal across batch sizes (kernel selection depends on the GEMM's M), so `predict` as a whole is reproducible for a
fixed `batch`, and `stitch_logits` for any `chunk`.

Scenes with no-data (`predict(valid=, nodata=, ...)`, csrc/scene_valid.hip: insar_scene_census / _gather_valid /
_finalize_valid): the valid pixels of every planned tile are counted on the device, only the tiles that hold enough of them are
run, invalid pixels enter the net as a fill value and leave with mask = conf = prob = 0 (DESIGN.md "Scenes with no-data").
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, _scene
from ._lib import InsarError, call, ptr
from .augment import D4_INVERSE, apply_table, check_tta, constant_table
from .distance import DistanceScratch, boundary_counts, boundary_iou
from .regions import DEFAULT_MAX_REGIONS, RegionScratch, label_regions
from .score import DEFAULT_MAX_PAIRS, OverlapScratch, match_regions

MAX_CLASSES = 8          # SC_MAX_K of csrc/scene.hip: the per-thread accumulators stay in registers up to here


def _check_geometry(H: int, W: int, tile: int, overlap: int) -> None:
    for name, v in (("H", H), ("W", W), ("tile", tile), ("overlap", overlap)):
        if int(v) != v:
            raise InsarError(f"plan_tiles: {name}={v!r} is not an integer")
    if tile < 16 or tile % 16:
        raise InsarError(f"tile={tile}: must be a positive multiple of 16 (the U-Net's four 2x2 poolings)")
    if not 0 <= overlap <= tile // 2:
        raise InsarError(f"overlap={overlap}: must lie in 0..tile // 2 = {tile // 2}")
    if H < tile or W < tile:
        raise InsarError(f"scene {H} x {W} is smaller than the tile {tile}: there is no padding path")


def _axis_origins(size: int, tile: int, stride: int) -> list:
    out = list(range(0, size - tile + 1, stride))
    if out[-1] != size - tile:
        out.append(size - tile)          # flush with the edge; overlaps its neighbours by more than `overlap`
    return out


def plan_tiles(H: int, W: int, tile: int, overlap: int) -> np.ndarray:
    """int32 [N, 2] tile origins (y0, x0), row-major over the tile grid. Host arithmetic only."""
    _check_geometry(H, W, tile, overlap)
    H, W, tile, overlap = int(H), int(W), int(tile), int(overlap)
    ys = _axis_origins(H, tile, tile - overlap)
    xs = _axis_origins(W, tile, tile - overlap)
    return np.array([(y, x) for y in ys for x in xs], dtype=np.int32).reshape(-1, 2)


def window_1d(tile: int, overlap: int) -> np.ndarray:
    """float32 [tile]: r(i) = min(i + 1, tile - i, overlap + 1) / (overlap + 1), the quotient the blend kernel forms."""
    if tile < 1 or not 0 <= overlap <= tile // 2:
        raise InsarError(f"window_1d: tile={tile}, overlap={overlap}: need 0 <= overlap <= tile // 2")
    i = np.arange(tile)
    m = np.minimum(np.minimum(i + 1, tile - i), overlap + 1)
    return m.astype(np.float32) / np.float32(overlap + 1)


def _check_origins(origins, H: int, W: int, tile: int) -> np.ndarray:
    o = origins.detach().cpu().numpy() if isinstance(origins, torch.Tensor) else np.asarray(origins)
    if o.ndim != 2 or o.shape[1] != 2 or o.shape[0] < 1 or not np.issubdtype(o.dtype, np.integer):
        raise InsarError(f"origins: expected an integer [N, 2] table, got {o.dtype} {o.shape}")
    if (o < 0).any() or (o[:, 0] + tile > H).any() or (o[:, 1] + tile > W).any():
        raise InsarError(f"origins: a {tile} x {tile} tile leaves the {H} x {W} scene")
    return np.ascontiguousarray(o, dtype=np.int32)


def _check_classes(K: int) -> None:
    if not 2 <= K <= MAX_CLASSES:
        raise InsarError(f"num_classes={K}: the scene kernels cover 2..{MAX_CLASSES} classes")


def _as_scene(scene, device: torch.device) -> torch.Tensor:
    """2-D uint8 / float32 numpy array or tensor -> contiguous device tensor (a host scene is copied once)."""
    if isinstance(scene, np.ndarray):
        if scene.dtype not in (np.uint8, np.float32):
            raise InsarError(f"scene dtype {scene.dtype}: uint8 or float32")
        if scene.ndim != 2:
            raise InsarError(f"scene must be 2-D [H, W], got {scene.ndim}-D")
        scene = torch.from_numpy(np.ascontiguousarray(scene))
    elif not isinstance(scene, torch.Tensor):
        raise InsarError(f"scene: numpy array or torch tensor, got {type(scene).__name__}")
    if scene.dtype not in (torch.uint8, torch.float32):
        raise InsarError(f"scene dtype {scene.dtype}: uint8 or float32")
    if scene.dim() != 2:
        raise InsarError(f"scene must be 2-D [H, W], got {scene.dim()}-D")
    if device.type != "cuda":
        raise InsarError("scene inference runs on a ROCm device (no CPU fallback)")
    return scene.detach().to(device).contiguous()


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _check_validity(who: str, H: int, W: int, is_u8: bool, tile: int, valid, nodata, min_valid, fill, norm):
    """The refusals of the no-data arguments, by name and before anything is copied to a device. Returns
    (valid as a uint8 [H, W] tensor wherever it lives, or None; nodata as a float, or None; min_valid; fill;
    (offset, scale) as floats, or None)."""
    if valid is not None:
        if isinstance(valid, np.ndarray):
            if valid.dtype != np.uint8 or valid.shape != (H, W):
                raise InsarError(f"{who}: valid must be a uint8 [{H}, {W}] numpy array or tensor, got {valid.dtype} {valid.shape}")
            valid = torch.from_numpy(np.ascontiguousarray(valid))
        _scene.check_map(who, "valid", valid, (torch.uint8,), shape=(H, W), of="the scene")
        valid = valid.detach()
    if nodata is not None:
        if is_u8:
            nodata = float(_scene.check_int(who, "nodata", nodata, 0, 255, integral_floats=True,
                                            expect="an integer in 0..255 for a uint8 scene"))
        elif not _is_number(nodata):
            raise InsarError(f"{who}: nodata={nodata!r}: a float for a float32 scene (nan: the non-finite pixels only)")
        else:
            nodata = float(nodata)
    min_valid = _scene.check_int(who, "min_valid", min_valid, 1, tile * tile, integral_floats=False)
    if not _is_number(fill) or not np.isfinite(fill):
        raise InsarError(f"{who}: fill={fill!r}: a finite float, the network input of an invalid pixel")
    if norm is not None:
        if is_u8:
            raise InsarError(f"{who}: norm is for float32 scenes: a uint8 scene gets the reference's transform")
        if not isinstance(norm, (tuple, list)) or len(norm) != 2 or not all(_is_number(v) for v in norm):
            raise InsarError(f"{who}: norm={norm!r}: a pair (offset, scale) of numbers")
        offset, scale = float(norm[0]), float(norm[1])
        if not np.isfinite(offset):
            raise InsarError(f"{who}: norm: offset={offset!r} is not finite")
        if not np.isfinite(scale) or scale == 0.0:
            raise InsarError(f"{who}: norm: scale={scale!r}: finite and not zero")
        norm = (offset, scale)
    return valid, nodata, min_valid, float(fill), norm


def _check_scene_args(who: str, scene, origins_dev, valid) -> None:
    if not isinstance(scene, torch.Tensor) or not isinstance(origins_dev, torch.Tensor) or not scene.is_cuda or not origins_dev.is_cuda:
        raise InsarError(f"{who}: scene and origins must be ROCm tensors (no CPU fallback)")
    if scene.dim() != 2 or scene.dtype not in (torch.uint8, torch.float32) or not scene.is_contiguous():
        raise InsarError(f"{who}: scene must be a contiguous 2-D uint8 or float32 tensor")
    if origins_dev.dtype != torch.int32 or origins_dev.dim() != 2 or origins_dev.shape[1] != 2 or not origins_dev.is_contiguous():
        raise InsarError(f"{who}: origins must be a contiguous int32 [n, 2] tensor")
    if valid is not None:
        _scene.check_map(who, "valid", valid, (torch.uint8,), shape=tuple(scene.shape), of="the scene")
        _scene.check_on_device(who, "valid", valid, like=scene)


def _scene_code(scene: torch.Tensor) -> int:
    return _lib.SCENE_U8 if scene.dtype == torch.uint8 else _lib.SCENE_F32


def gather_tiles(scene: torch.Tensor, origins_dev: torch.Tensor, tile: int, out: Optional[torch.Tensor] = None, *, valid=None,
                 nodata=None, fill: float = 0.0, norm=None) -> torch.Tensor:
    """float32 [n, 1, tile, tile] <- the tiles of a device scene [H, W] at the int32 device table `origins_dev` [n, 2]
    (every tile inside the scene). uint8 scenes are normalised like `data.reference_transforms`, float32 ones copied, or
    taken through x = (v - offset) * scale with `norm` = (offset, scale). With `valid` (a uint8 [H, W] device map, 0 = not
    observed) or `nodata` every invalid pixel (see `ScenePredictor.predict`) comes out as `fill`. With all four at their
    defaults this is insar_scene_gather; otherwise insar_scene_gather_valid."""
    _check_scene_args("gather_tiles", scene, origins_dev, valid)
    plain = valid is None and nodata is None and norm is None and type(fill) is float and fill == 0.0
    if not plain:
        _, nodata, _, fill, norm = _check_validity("gather_tiles", scene.shape[0], scene.shape[1], scene.dtype == torch.uint8, tile,
                                                   valid, nodata, 1, fill, norm)
        plain = valid is None and nodata is None and norm is None and fill == 0.0
    n = origins_dev.shape[0]
    if out is None:
        out = torch.empty(n, 1, tile, tile, dtype=torch.float32, device=scene.device)
    if plain:
        call("insar_scene_gather", ptr(scene), _scene_code(scene), scene.shape[0], scene.shape[1], ptr(origins_dev), n, tile,
             ptr(out), _lib.stream_ptr())
    else:
        offset, scale = norm if norm is not None else (0.0, 1.0)
        call("insar_scene_gather_valid", ptr(scene), _scene_code(scene), scene.shape[0], scene.shape[1], ptr(valid),
             int(nodata is not None), 0.0 if nodata is None else nodata, fill, int(norm is not None), offset, scale,
             ptr(origins_dev), n, tile, ptr(out), _lib.stream_ptr())
    return out


def tile_census(scene: torch.Tensor, origins_dev: torch.Tensor, tile: int, *, valid=None, nodata=None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [n] on the device <- the number of valid pixels (see `ScenePredictor.predict`) of each tile of a device scene
    [H, W] at the int32 device table `origins_dev` [n, 2]. One launch (insar_scene_census), nothing read back."""
    _check_scene_args("tile_census", scene, origins_dev, valid)
    _, nodata, _, _, _ = _check_validity("tile_census", scene.shape[0], scene.shape[1], scene.dtype == torch.uint8, tile, valid, nodata,
                                         1, 0.0, None)
    n = origins_dev.shape[0]
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=scene.device)
    call("insar_scene_census", ptr(scene), _scene_code(scene), scene.shape[0], scene.shape[1], ptr(valid), int(nodata is not None),
         0.0 if nodata is None else nodata, ptr(origins_dev), n, tile, ptr(out), _lib.stream_ptr())
    return out


def select_tiles(counts, min_valid: int = 1) -> np.ndarray:
    """The indices, ascending, of the tiles whose census is at least `min_valid`: the tiles that are run. Host arithmetic
    only."""
    c = np.asarray(counts)
    if c.ndim != 1 or not np.issubdtype(c.dtype, np.integer):
        raise InsarError(f"select_tiles: counts must be a 1-D integer array, got {c.dtype} {c.shape}")
    min_valid = _scene.check_int("select_tiles", "min_valid", min_valid, 1, integral_floats=False)
    return np.flatnonzero(c >= min_valid)


def _blend(logits: torch.Tensor, origins: np.ndarray, origins_dev: torch.Tensor, first: int, K: int, tile: int, overlap: int,
           acc: torch.Tensor, wsum: torch.Tensor) -> None:
    """Add tiles first .. first + n - 1 of the table (n = logits.shape[0]) into acc / wsum."""
    n = logits.shape[0]
    if tuple(logits.shape) != (n, K, tile, tile):
        raise InsarError(f"logits {tuple(logits.shape)}: expected ({n}, {K}, {tile}, {tile})")
    lg = logits.detach()
    if lg.dtype != torch.float32 or not lg.is_contiguous():
        lg = lg.float().contiguous()
    o = origins[first:first + n]
    H, W = wsum.shape
    call("insar_scene_blend", ptr(lg), ptr(origins_dev) + 8 * first, n, K, tile, overlap, ptr(acc), ptr(wsum), H, W,
         int(o[:, 0].min()), int(o[:, 0].max()) + tile, int(o[:, 1].min()), int(o[:, 1].max()) + tile, _lib.stream_ptr())


def _finalize(acc: torch.Tensor, wsum: torch.Tensor, return_prob: bool) -> Dict[str, torch.Tensor]:
    K, H, W = acc.shape
    dev = acc.device
    out = {"mask": torch.empty(H, W, dtype=torch.uint8, device=dev), "conf": torch.empty(H, W, dtype=torch.float32, device=dev)}
    if return_prob:
        out["prob"] = torch.empty(K, H, W, dtype=torch.float32, device=dev)
    call("insar_scene_finalize", ptr(acc), ptr(wsum), K, H, W, ptr(out.get("prob")), ptr(out["mask"]), ptr(out["conf"]),
         _lib.stream_ptr())
    return out


def _finalize_valid(acc: torch.Tensor, wsum: torch.Tensor, return_prob: bool, scene: torch.Tensor, valid, nodata) -> Dict[str, torch.Tensor]:
    """`_finalize` with prob = mask = conf = 0 at the pixels that are invalid or that no tile covered, and "valid"."""
    K, H, W = acc.shape
    dev = acc.device
    out = {"mask": torch.empty(H, W, dtype=torch.uint8, device=dev), "conf": torch.empty(H, W, dtype=torch.float32, device=dev),
           "valid": torch.empty(H, W, dtype=torch.uint8, device=dev)}
    if return_prob:
        out["prob"] = torch.empty(K, H, W, dtype=torch.float32, device=dev)
    call("insar_scene_finalize_valid", ptr(acc), ptr(wsum), K, H, W, ptr(scene), _scene_code(scene), ptr(valid), int(nodata is not None),
         0.0 if nodata is None else nodata, ptr(out.get("prob")), ptr(out["mask"]), ptr(out["conf"]), ptr(out["valid"]),
         _lib.stream_ptr())
    return out


def _accumulators(K: int, H: int, W: int, device: torch.device):
    buf = torch.empty(K + 1, H, W, dtype=torch.float32, device=device)      # one allocation, one clear per scene
    return buf, buf[:K], buf[K]


def stitch_logits(logits: torch.Tensor, origins, H: int, W: int, tile: int, overlap: int, chunk: Optional[int] = None,
                  return_prob: bool = True) -> Dict[str, torch.Tensor]:
    """The blend + finalize stage alone: logits [N, K, tile, tile] of the tiles at `origins` [N, 2] (index order = blend
    order) -> {"mask", "conf"[, "prob"]}, fed to the blend kernel `chunk` tiles at a time (None: all at once). The result
    does not depend on `chunk`, bit for bit."""
    _check_geometry(H, W, tile, overlap)
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        raise InsarError("stitch_logits: logits must be a ROCm tensor (no CPU fallback)")
    if logits.dim() != 4:
        raise InsarError(f"stitch_logits: logits must be [N, K, tile, tile], got {tuple(logits.shape)}")
    N, K = logits.shape[0], logits.shape[1]
    _check_classes(K)
    o = _check_origins(origins, H, W, tile)
    if o.shape[0] != N:
        raise InsarError(f"stitch_logits: {N} tiles of logits, {o.shape[0]} origins")
    chunk = N if chunk is None else int(chunk)
    if chunk < 1:
        raise InsarError(f"stitch_logits: chunk={chunk}")
    with torch.no_grad():
        o_dev = torch.from_numpy(o).to(logits.device)
        buf, acc, wsum = _accumulators(K, H, W, logits.device)
        buf.zero_()
        for i in range(0, N, chunk):
            _blend(logits[i:i + chunk], o, o_dev, i, K, tile, overlap, acc, wsum)
        return _finalize(acc, wsum, return_prob)


class ScenePredictor:
    """Tiled prediction of a whole scene with any net of this package (1-channel input, logits [n, K, tile, tile]).

        pred = ScenePredictor(net, tile=256, overlap=32, batch=16, num_classes=2)
        out = pred.predict(scene)                 # scene: 2-D uint8 / float32, numpy or torch, host or device
        out["mask"]  uint8 [H, W]   class map        out["conf"]  float32 [H, W]  its probability
        out["prob"]  float32 [K, H, W]               (return_prob=True)

    uint8 scenes are normalised as the reference's data_transforms do (v / 255, then (x - 0.5) / 0.5); float32 scenes are
    taken as already normalised. Works on the current stream; the tile batch, the origin table and the accumulators are
    kept between calls with the same scene size (the outputs are fresh tensors every call).

    `tta` = 2, 4 or 8 averages the class probabilities over the D4 ops 0 .. tta - 1 (augment.py: 2 adds the horizontal flip, 4
    the flips, 8 all flips and rotations): per batch and op, in ascending op order, the tiles are transformed
    (insar_aug_apply), the net runs, its float32 logits are transformed back with the inverse op and blended at the same
    origins; the blend adds into acc / wsum, so finalize returns the mean over ops. tta = 1 launches none of this. For a
    fixed `batch` and `tta` the output is bitwise reproducible.

        det = pred.detect(scene, min_area=20, min_conf=0.6)      # predict + regions.label_regions on its mask / conf
        det["labels"] int32 [H, W]   det["regions"] host table   det["count"] N   det["mask_clean"] uint8 [H, W]

        ev = pred.evaluate(scene, gt_mask, iou_threshold=0.5, min_area=20)      # detect + the score against a ground truth
        ev["score"]["overall"]["pq"]   ev["score"]["gt_match"]   ev["gt_labels"] int32 [H, W]   ev["gt_regions"]"""

    def __init__(self, model: torch.nn.Module, tile: int = 256, overlap: int = 32, batch: int = 16, num_classes: int = 2,
                 tta: int = 1):
        _check_geometry(tile, tile, tile, overlap)
        self.tta = check_tta(tta)
        _check_classes(num_classes)
        if int(batch) != batch or batch < 1:
            raise InsarError(f"batch={batch!r}: a positive integer")
        self.model, self.tile, self.overlap, self.batch, self.num_classes = model, int(tile), int(overlap), int(batch), int(num_classes)
        self._geom: dict = {}            # (H, W, device) -> (origins, origins_dev, buf, acc, wsum)
        self._tiles: dict = {}           # device -> float32 [batch, 1, tile, tile]
        self._tta: dict = {}             # device -> (tables int32 [8, batch, 4], tiles' and logits' transformed copies)
        self._kept: dict = {}            # (H, W, device) -> (the run tiles' origins int32 [N, 2], the census int32 [N])
        self._cache: dict = {}           # (Scratch class, key, device) -> the scratch of a scene tool

    def _buffers(self, H: int, W: int, device: torch.device):
        key = (H, W, device)
        if key not in self._geom:
            origins = plan_tiles(H, W, self.tile, self.overlap)
            self._geom[key] = (origins, torch.from_numpy(origins).to(device)) + _accumulators(self.num_classes, H, W, device)
        if device not in self._tiles:
            self._tiles[device] = torch.empty(self.batch, 1, self.tile, self.tile, dtype=torch.float32, device=device)
        return self._geom[key] + (self._tiles[device],)

    def release(self) -> None:
        """Drop the cached buffers (they are scene-sized)."""
        self._geom.clear()
        self._tiles.clear()
        self._tta.clear()
        self._kept.clear()
        self._cache.clear()

    def _scratch(self, cls, device, *key):
        """The scratch of class `cls` for `key` on `device`, built on first use and kept until `release()`; None for a key the
        class does not take, so that the tool itself refuses the argument by name."""
        k = (cls, key, device)
        if k not in self._cache:
            scratch = cls.build(device, *key)
            if scratch is None:
                return None
            self._cache[k] = scratch
        return self._cache[k]

    def _cached(self, cls) -> list:
        """The scratch objects of class `cls` that are held now."""
        return [s for (c, _, _), s in self._cache.items() if c is cls]

    def _tta_buffers(self, device: torch.device):
        if device not in self._tta:
            tables = constant_table([op for op in range(8) for _ in range(self.batch)], device).view(8, self.batch, 4)
            self._tta[device] = (tables, torch.empty(self.batch, 1, self.tile, self.tile, dtype=torch.float32, device=device),
                                 torch.empty(self.batch, self.num_classes, self.tile, self.tile, dtype=torch.float32, device=device))
        return self._tta[device]

    def _forward_tta(self, x: torch.Tensor, op: int, n: int, bufs) -> torch.Tensor:
        """Logits of the n tiles `x` seen through D4 op `op`, brought back to the tiles' own orientation."""
        tables, xt, lt = bufs
        apply_table(x, None, tables[op, :n], out=(xt[:n], None))
        lg = self.model(xt[:n]).detach()
        if tuple(lg.shape) != (n, self.num_classes, self.tile, self.tile):
            raise InsarError(f"logits {tuple(lg.shape)}: expected ({n}, {self.num_classes}, {self.tile}, {self.tile})")
        if lg.dtype != torch.float32 or not lg.is_contiguous():
            lg = lg.float().contiguous()
        apply_table(lg, None, tables[D4_INVERSE[op], :n], out=(lt[:n], None))
        return lt[:n]

    def _kept_buffers(self, H: int, W: int, device: torch.device, N: int):
        key = (H, W, device)
        if key not in self._kept:
            self._kept[key] = (torch.empty(N, 2, dtype=torch.int32, device=device), torch.empty(N, dtype=torch.int32, device=device))
        return self._kept[key]

    @torch.no_grad()
    def predict(self, scene, return_prob: bool = False, *, valid=None, nodata=None, min_valid: int = 1, fill: float = 0.0,
                norm=None) -> Dict[str, torch.Tensor]:
        """The tiled prediction of `scene`. With `valid` (uint8 [H, W], numpy or tensor, copied to the device once; 0 = not
        observed) or `nodata` the scene has no-data, and a pixel is VALID iff its byte of `valid` is non-zero (None: every
        one), its value is not `nodata` (an exact compare: an integer in 0..255 for a uint8 scene, a float for a float32 one)
        and, in a float32 scene, it is finite (nodata=float("nan"): the non-finite pixels only). Then only the tiles of
        `plan_tiles` that hold at least `min_valid` (1..tile^2) valid pixels are run, in their row-major order; inside them an
        invalid pixel enters the net as `fill` (finite, in the net's input domain; 0.0 is mid-grey after the reference's
        normalisation); an invalid pixel, and a valid one that no run tile covers (min_valid > 1 only), has mask = 0, conf = 0
        and prob = 0, and the result gains "valid" (uint8 [H, W], 1 = valid and covered), "tiles_total", "tiles_run" and
        "tile_valid" (host int32 [N], the valid pixels of every planned tile). No run tile: no forward, all zero, no error.
        `norm` = (offset, scale) takes a float32 scene through x = (v - offset) * scale on the way into the tiles (refused
        for uint8 scenes); alone it selects neither the census nor the masking. With all five at their defaults nothing of
        this runs."""
        shape = tuple(getattr(scene, "shape", ()))
        if len(shape) == 2:
            _check_geometry(shape[0], shape[1], self.tile, self.overlap)       # refuse before anything is copied
        masked = valid is not None or nodata is not None
        if len(shape) == 2:              # anything else is `_as_scene`'s to refuse
            is_u8 = getattr(scene, "dtype", None) in (np.uint8, torch.uint8)
            valid, nodata, min_valid, fill, norm = _check_validity("predict", shape[0], shape[1], is_u8, self.tile, valid, nodata,
                                                                   min_valid, fill, norm)
        try:
            device = next(self.model.parameters()).device
        except StopIteration:
            raise InsarError("ScenePredictor: the model has no parameters") from None
        sc = _as_scene(scene, device)
        H, W = sc.shape
        K, T = self.num_classes, self.tile
        origins, o_dev, buf, acc, wsum, tiles = self._buffers(H, W, device)
        N = origins.shape[0]
        extra = {}
        if masked:
            if valid is not None:
                valid = valid.to(device)
            kept_dev, counts_dev = self._kept_buffers(H, W, device, N)
            tile_census(sc, o_dev, T, valid=valid, nodata=nodata, out=counts_dev)
            tile_valid = counts_dev.cpu().numpy()                          # the one read-back of a masked predict
            kept = select_tiles(tile_valid, min_valid)
            extra = {"tiles_total": int(N), "tiles_run": int(kept.size), "tile_valid": tile_valid}
            origins, o_dev, N = np.ascontiguousarray(origins[kept]), kept_dev, int(kept.size)
            if N:
                o_dev[:N].copy_(torch.from_numpy(origins))
        gather_kw = {} if not masked and norm is None else dict(valid=valid, nodata=nodata, fill=fill, norm=norm)
        tta_bufs = self._tta_buffers(device) if self.tta > 1 else None
        was_training = self.model.training
        self.model.eval()
        try:
            buf.zero_()
            for i in range(0, N, self.batch):
                n = min(self.batch, N - i)
                x = gather_tiles(sc, o_dev[i:i + n], T, out=tiles[:n], **gather_kw)
                if self.tta == 1:
                    _blend(self.model(x), origins, o_dev, i, K, T, self.overlap, acc, wsum)
                    continue
                for op in range(self.tta):
                    _blend(self._forward_tta(x, op, n, tta_bufs), origins, o_dev, i, K, T, self.overlap, acc, wsum)
        finally:
            self.model.train(was_training)
        if not masked:
            return _finalize(acc, wsum, return_prob)
        out = _finalize_valid(acc, wsum, return_prob, sc, valid, nodata)
        out.update(extra)
        return out

    def detect(self, scene, return_prob: bool = False, outlines: bool = False, skeletons: bool = False,
               max_iterations: int = 32, measure: Optional[dict] = None, simplify: Optional[float] = None, split=None,
               sieve=None, valid=None, nodata=None, min_valid: int = 1, fill: float = 0.0, norm=None, hysteresis=None,
               contours: Optional[dict] = None, **region_kwargs) -> dict:
        """`predict(scene)` followed by `label_regions(out["mask"], out["conf"], **region_kwargs)`: the predict outputs
        unchanged, plus "labels", "regions", "count" and the cleaned class map under "mask_clean". With `outlines=True` also
        "outlines" = `outlines.region_outlines(out["labels"])` with the connectivity the regions were labelled with, and
        out["regions"]["perimeter"], the crack length of each region over all of its rings. With `simplify` = a tolerance in
        pixels next to `outlines=True`, "outlines" is instead `simplify.simplify_outlines` of the rings traced with
        corners_only=False, with out["labels"] as the label map, so touching regions share their border vertex for vertex; the
        untouched trace is not kept, and the perimeter, which comes from `edges`, is the same. With `skeletons=True` also
        "skeleton" = the kinds map of `skeletons.thin_regions(out["labels"], max_iterations=max_iterations)`, "skeleton_converged",
        and out["regions"]["length"], ["mean_width"], ["max_width"], ["orientation"], ["n_end"], ["n_junction"]. With `measure` =
        {name: raster} or {name: (raster, kwargs)} also "stats"[name] = `zonal.region_stats(out["labels"], raster,
        count=out["count"], max_regions=..., **kwargs)`, rows aligned with out["regions"]["id"]: a raster is [H, W] or
        [C, H, W], float32, uint8 or int32, numpy or tensor (a host raster is copied once); the string "input" stands for the
        scene that was predicted (a uint8 scene is measured as its byte values). With `split` = True, a number (`min_depth`) or a
        dict of `split.split_regions` keywords, the regions are cut along the necks of their distance map right after
        `label_regions`: the pieces replace "labels", "regions" and "count" (the table gains parent, peak, peak_y, peak_x and
        saddle), "split_rounds" and "split_converged" are added, "mask_clean" is unchanged, and outlines, skeletons and
        `measure` run on the pieces. With None nothing of it runs. With `sieve` = an int, a {class: int} dict or a sequence
        (`min_area` of `sieve.sieve_regions`), or a dict of its keywords (`connectivity` and `max_regions` default to
        detect's own), the predicted class map is sieved right after `predict`: small regions are absorbed by their largest
        neighbour and small holes fill, `label_regions` and everything after it run on the cleaned map, "mask" stays the raw
        prediction, and "mask_sieved", "sieve_changed_pixels", "sieve_absorbed", "sieve_rounds" and "sieve_converged" are
        added. "conf" is not rewritten: a filled pixel carries the confidence of the class it had. With None nothing of it
        runs. `valid`, `nodata`, `min_valid`, `fill` and `norm` go to `predict`: an invalid pixel is class 0, hence background
        for the regions. With `hysteresis` = (low, high) or a dict of `hysteresis.hysteresis_regions` keywords, the sites are
        grown from confident seeds instead: `predict` computes the class probabilities ("prob" is in the result only if
        `return_prob`), `hysteresis_regions(prob, low, high, valid=out.get("valid"), ...)` with detect's `connectivity`,
        `min_area` and `max_regions` replaces the `label_regions` call, "labels", "regions" (which gain n_seed, peak, peak_y and
        peak_x) and "count" come from it, "mask_clean" is its mask, "conf_hysteresis" its candidate plane,
        "hysteresis_candidates" the components before the seed rule, and "mask" and "conf" stay the raw prediction. `min_conf`
        and `sieve` are refused next to it: the two thresholds replace the one, and a sieved arg-max map and a low-threshold
        map are different maps. With None nothing of it runs. With `contours` = a dict of `contours.contour_lines` keywords
        (`levels` is needed) plus `raster` (None) and `plane` (1), also "contours" = `contour_lines(raster, levels, ...)`:
        `raster` None contours probability plane `plane` (`predict` then computes the probabilities; "prob" is in the result
        only if `return_prob`), else a float32, uint8 or int32 [H, W] raster on the scene grid, numpy or tensor (a host raster
        is copied once); the "valid" plane of a masked predict is handed on, so that lines end beside no-data. With `smooth` =
        a Gaussian sigma in pixels (0 < sigma <= 5) in that dict the contoured raster first goes through
        `focal.smooth_raster(raster, gaussian_taps(sigma), valid=, return_valid=True)` and that valid plane goes to
        `contour_lines`; without it not one operation changes. With `simplify` = a tolerance in pixels (0 .. 1024) in that
        dict "contours" is instead `simplify_contours` of those lines; without it not one operation changes either. With None
        nothing of it runs."""
        if measure is not None and not isinstance(measure, dict):
            raise InsarError(f"measure: a dict of name -> raster or (raster, kwargs), got {type(measure).__name__}")
        if hysteresis is not None:
            hyst_kw = self._hysteresis_kwargs(hysteresis, sieve, region_kwargs)
        need_prob = hysteresis is not None
        if contours is not None:
            contour_kw = self._contour_kwargs(contours)
            need_prob = need_prob or contour_kw["raster"] is None
        out = dict(self.predict(scene, return_prob=return_prob or need_prob, valid=valid, nodata=nodata,
                                min_valid=min_valid, fill=fill, norm=norm))
        if contours is not None:
            self._contour(out, contour_kw)                                   # before `_grow` takes "prob" out
            if need_prob and hysteresis is None and not return_prob:
                del out["prob"]
        H, W = out["mask"].shape
        max_regions = region_kwargs.get("max_regions", DEFAULT_MAX_REGIONS)
        if hysteresis is not None:
            self._grow(out, hyst_kw, return_prob)
        else:
            class_map = out["mask"] if sieve is None else self._sieve(out, sieve, region_kwargs.get("connectivity", 8), max_regions)
            reg = label_regions(class_map, out["conf"], scratch=self._scratch(RegionScratch, out["mask"].device, H, W, max_regions),
                                **region_kwargs)
            out.update(labels=reg["labels"], regions=reg["regions"], count=reg["count"], mask_clean=reg["mask"])
        if split is not None and split is not False:
            self._split(out, split, max_regions)
        if simplify is not None and not outlines:
            raise InsarError("detect: simplify needs outlines=True")
        if outlines:
            self._trace(out, region_kwargs.get("connectivity", 8), simplify)
        if skeletons:
            self._thin(out, max_iterations, max_regions)
        if measure is not None:
            self._measure(out, scene, measure, max_regions)
        return out

    @staticmethod
    def _contour_kwargs(contours) -> dict:
        """The keywords of `contour_lines` plus "raster" and "plane" from detect's `contours`; refused before `predict` runs."""
        if not isinstance(contours, dict) or "levels" not in contours:
            raise InsarError(f"contours: a dict of contour_lines keywords with 'levels' (and 'raster', 'plane'), got {contours!r}")
        kw = dict(contours)
        for name in ("valid", "scratch"):
            if name in kw:
                raise InsarError(f"contours: {name!r} is detect's to give")
        kw.setdefault("raster", None)
        kw.setdefault("plane", 1)
        if kw.get("smooth") is not None:
            sigma = kw["smooth"]
            if (isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating))
                    or not 0 < sigma <= 5):               # NaN compares false
                raise InsarError(f"contours: smooth={sigma!r}: a Gaussian sigma in pixels, 0 < sigma <= 5")
        if kw.get("simplify") is not None:
            from .contours import check_tolerance
            check_tolerance("contours", "simplify", kw["simplify"])
        return kw

    def _contour(self, out: dict, kw: dict) -> None:
        """`contour_lines` of a probability plane or of the caller's raster, with the valid plane of a masked predict."""
        from .contours import DEFAULT_MAX_LINES, DEFAULT_MAX_VERTICES, ContourScratch, contour_lines
        kw = dict(kw)
        raster, plane, sigma = kw.pop("raster"), kw.pop("plane"), kw.pop("smooth", None)
        tolerance = kw.pop("simplify", None)
        dev = out["mask"].device
        if raster is None:
            K = out["prob"].shape[0]
            plane = _scene.check_int("contours", "plane", plane, 0, K - 1, integral_floats=False)
            raster = out["prob"][plane]
        else:
            if isinstance(raster, np.ndarray):
                raster = torch.from_numpy(np.ascontiguousarray(raster))
            if not isinstance(raster, torch.Tensor):
                raise InsarError(f"contours: raster must be a numpy array or a torch tensor, got {type(raster).__name__}")
            raster = raster.detach().to(dev).contiguous()
        levels = kw.pop("levels")
        n_levels = len(levels) if isinstance(levels, (list, tuple, np.ndarray)) else 1
        scratch = None
        if raster.dim() == 2:
            scratch = self._scratch(ContourScratch, dev, raster.shape[0], raster.shape[1], n_levels,
                                    kw.get("max_lines", DEFAULT_MAX_LINES), kw.get("max_vertices", DEFAULT_MAX_VERTICES))
        valid = out.get("valid")
        if sigma is not None:                                                # the valid plane of the smoothing ends the lines
            from .focal import gaussian_taps, smooth_raster
            raster, valid = smooth_raster(raster, gaussian_taps(float(sigma)), valid=valid, return_valid=True)
        out["contours"] = contour_lines(raster, levels, valid=valid, scratch=scratch, **kw)
        if tolerance is not None:
            from .contours import simplify_contours
            out["contours"] = simplify_contours(out["contours"], tolerance=tolerance)

    @staticmethod
    def _hysteresis_kwargs(hysteresis, sieve, region_kwargs: dict) -> dict:
        """The keywords of `hysteresis_regions` from detect's `hysteresis` and region keywords; refused before `predict` runs."""
        if isinstance(hysteresis, dict):
            kw = dict(hysteresis)
            if "low" not in kw or "high" not in kw:
                raise InsarError("hysteresis: a dict of hysteresis_regions keywords needs 'low' and 'high'")
        elif isinstance(hysteresis, (tuple, list)) and len(hysteresis) == 2:
            kw = {"low": hysteresis[0], "high": hysteresis[1]}
        else:
            raise InsarError(f"hysteresis: (low, high) or a dict of hysteresis_regions keywords, got {hysteresis!r}")
        for name in ("score", "valid", "scratch"):
            if name in kw:
                raise InsarError(f"hysteresis: {name!r} is detect's to give")
        if "min_conf" in region_kwargs:
            raise InsarError("detect: min_conf next to hysteresis: the two thresholds replace it (low is the cut on the extent)")
        if sieve is not None:
            raise InsarError("detect: sieve next to hysteresis: a sieved arg-max map and a low-threshold map are different maps, "
                             "and their combination is not defined")
        for name, v in region_kwargs.items():
            if name not in ("connectivity", "min_area", "max_regions"):
                raise InsarError(f"detect: {name!r} next to hysteresis: connectivity, min_area and max_regions are handed to it")
            kw.setdefault(name, v)
        return kw

    def _grow(self, out: dict, kw: dict, return_prob: bool) -> None:
        """`hysteresis_regions` of out["prob"] in place of `label_regions`; its results go into `out`."""
        from .hysteresis import HysteresisScratch, hysteresis_regions
        prob = out["prob"] if return_prob else out.pop("prob")
        _, H, W = prob.shape
        scratch = self._scratch(HysteresisScratch, prob.device, H, W, kw.get("max_regions", DEFAULT_MAX_REGIONS))
        hy = hysteresis_regions(prob, kw.pop("low"), kw.pop("high"), valid=out.get("valid"), scratch=scratch, **kw)
        out.update(labels=hy["labels"], regions=hy["regions"], count=hy["count"], mask_clean=hy["mask"],
                   conf_hysteresis=hy["conf"], hysteresis_candidates=hy["candidates"])

    def _sieve(self, out: dict, sieve, connectivity: int, max_regions: int) -> torch.Tensor:
        """The sieved class map of out["mask"]; the sieve's figures go into `out`."""
        from .sieve import DEFAULT_MAX_PAIRS, SieveScratch, sieve_regions
        if isinstance(sieve, dict) and any(isinstance(k, str) for k in sieve):
            kw = dict(sieve)
            if "min_area" not in kw:
                raise InsarError("sieve: a dict of sieve_regions keywords needs 'min_area'")
        elif isinstance(sieve, (dict, list, tuple, np.ndarray, int, float, np.integer, np.floating)) and not isinstance(sieve, bool):
            kw = {"min_area": sieve}
        else:
            raise InsarError(f"sieve: an int, a {{class: int}} dict or a sequence (min_area), or a dict of sieve_regions keywords, "
                             f"got {sieve!r}")
        for name in ("mask", "scratch"):
            if name in kw:
                raise InsarError(f"sieve: {name!r} is detect's to give")
        kw.setdefault("connectivity", connectivity)
        kw.setdefault("max_regions", max_regions)
        H, W = out["mask"].shape
        scratch = self._scratch(SieveScratch, out["mask"].device, H, W, kw["max_regions"], kw.get("max_pairs", DEFAULT_MAX_PAIRS),
                                kw.get("max_rounds", 64))
        sv = sieve_regions(out["mask"], scratch=scratch, **kw)
        out.update(mask_sieved=sv["mask"], sieve_changed_pixels=sv["changed_pixels"], sieve_absorbed=sv["absorbed"],
                   sieve_rounds=sv["rounds"], sieve_converged=sv["converged"])
        if "changed" in sv:
            out["sieve_changed"] = sv["changed"]
        return sv["mask"]

    def _split(self, out: dict, split, max_regions: int) -> None:
        from .split import DEFAULT_MAX_PAIRS, SplitScratch, split_regions
        if split is True:
            kw = {}
        elif isinstance(split, dict):
            kw = dict(split)
        elif isinstance(split, (int, float, np.integer, np.floating)) and not isinstance(split, bool):
            kw = {"min_depth": split}
        else:
            raise InsarError(f"split: True, a number (min_depth) or a dict of split_regions keywords, got {split!r}")
        for name in ("mask", "conf", "scratch"):
            if name in kw:
                raise InsarError(f"split: {name!r} is detect's to give")
        kw.setdefault("max_regions", max_regions)
        H, W = out["labels"].shape
        scratch = self._scratch(SplitScratch, out["labels"].device, H, W, kw["max_regions"], kw.get("max_pairs", DEFAULT_MAX_PAIRS),
                                kw.get("max_rounds", 64))
        # with hysteresis the labels reach below the arg-max boundary: their confidence is the candidate plane
        sp = split_regions(out["labels"], mask=out["mask_clean"], conf=out.get("conf_hysteresis", out["conf"]), scratch=scratch, **kw)
        out.update(labels=sp["labels"], regions=sp["regions"], count=sp["count"], split_rounds=sp["rounds"],
                   split_converged=sp["converged"])

    def _measure(self, out: dict, scene, measure: dict, max_regions: int) -> None:
        from .zonal import ZonalScratch, region_stats
        dev = out["labels"].device
        out["stats"] = {}
        for name, spec in measure.items():
            raster, kw = spec if isinstance(spec, tuple) else (spec, {})
            if isinstance(raster, str):
                if raster != "input":
                    raise InsarError(f"measure[{name!r}]: the only raster named by a string is \"input\", got {raster!r}")
                raster = scene
            if isinstance(raster, np.ndarray):
                raster = torch.from_numpy(np.ascontiguousarray(raster))
            if not isinstance(raster, torch.Tensor):
                raise InsarError(f"measure[{name!r}]: numpy array or torch tensor, got {type(raster).__name__}")
            raster = raster.detach().to(dev).contiguous()
            scratch = self._scratch(ZonalScratch, dev, max_regions, kw.get("bins", 0), raster.shape[0] if raster.dim() == 3 else 1)
            out["stats"][name] = region_stats(out["labels"], raster, count=out["count"], max_regions=max_regions, scratch=scratch, **kw)

    def _thin(self, out: dict, max_iterations: int, max_regions: int) -> None:
        from .skeletons import SkeletonScratch, thin_regions
        H, W = out["labels"].shape
        sk = thin_regions(out["labels"], max_iterations=max_iterations, max_regions=max_regions,
                          scratch=self._scratch(SkeletonScratch, out["labels"].device, H, W, max_iterations, max_regions))
        out["skeleton"], out["skeleton_converged"] = sk["skeleton"], sk["converged"]
        # region ids are labels: row id - 1 of the table; a kept region always has a pixel, hence a record
        rows = np.asarray(out["regions"]["id"], dtype=np.int64) - 1
        for f in ("length", "mean_width", "max_width", "orientation", "n_end", "n_junction"):
            out["regions"][f] = sk["table"][f][rows]

    def _trace(self, out: dict, connectivity: int, tolerance: Optional[float] = None) -> None:
        """The outlines of out["labels"]; with a tolerance, traced vertex by vertex and simplified against the label map."""
        from .outlines import DEFAULT_MAX_EDGES, DEFAULT_MAX_RINGS, DEFAULT_MAX_VERTICES, OutlineScratch, perimeters, region_outlines
        from .simplify import simplify_outlines
        H, W = out["labels"].shape
        scratch = self._scratch(OutlineScratch, out["labels"].device, H, W, DEFAULT_MAX_RINGS, DEFAULT_MAX_VERTICES, DEFAULT_MAX_EDGES)
        out["outlines"] = region_outlines(out["labels"], connectivity=connectivity, corners_only=tolerance is None, scratch=scratch)
        if tolerance is not None:
            out["outlines"] = simplify_outlines(out["outlines"], out["labels"], tolerance=tolerance)
        out["regions"]["perimeter"] = perimeters(out["outlines"]["rings"], out["regions"]["id"])

    def evaluate(self, scene, gt_mask, *, iou_threshold: float = 0.5, gt_min_area: int = 1, max_pairs: int = DEFAULT_MAX_PAIRS,
                 boundary_distance: Optional[int] = None, measure: Optional[dict] = None, sieve=None, valid=None, nodata=None,
                 min_valid: int = 1, fill: float = 0.0, norm=None, hysteresis=None, **region_kwargs) -> dict:
        """`detect(scene, **region_kwargs)`, then `label_regions` of the ground-truth class map (`gt_mask` uint8 [H, W], numpy
        or tensor, copied to the device once; 255 = ignore, labelled as background) with the same connectivity and
        `min_area=gt_min_area`, then `score.match_regions` with `void=gt_mask, void_value=255`: the detect outputs unchanged,
        plus "score" (the match result), "gt_labels", "gt_regions" and "gt_count". With `boundary_distance` = d (an integer
        >= 0) the score gains "boundary" = {"distance", "counts", "iou", "mean_iou"}: `distance.boundary_counts` of
        "mask_clean" against `gt_mask` (void 255) at d pixels, and `boundary_iou` of them; with None nothing of it runs.
        `measure`, `sieve` and `hysteresis` go to `detect`: they shape the prediction only, never the ground truth. `valid`, `nodata`,
        `min_valid`, `fill` and `norm` go to `predict`; where its "valid" is 0 the ground truth is set to 255 before anything
        else, so that a ground-truth object wholly in no-data is no region at all (neither a miss nor a match), and one partly
        in it is scored on its valid part."""
        out = self.detect(scene, measure=measure, sieve=sieve, valid=valid, nodata=nodata, min_valid=min_valid, fill=fill, norm=norm,
                          hysteresis=hysteresis, **region_kwargs)
        dev = out["mask"].device
        H, W = out["mask"].shape
        gt = torch.from_numpy(np.ascontiguousarray(gt_mask)) if isinstance(gt_mask, np.ndarray) else gt_mask
        if not isinstance(gt, torch.Tensor) or gt.dtype != torch.uint8 or tuple(gt.shape) != (H, W):
            raise InsarError(f"evaluate: gt_mask must be a uint8 [{H}, {W}] numpy array or tensor, got "
                             f"{getattr(gt, 'dtype', type(gt).__name__)} {tuple(getattr(gt, 'shape', ()))}")
        gt = gt.detach().to(dev).contiguous()
        if "valid" in out:
            gt = torch.where(out["valid"] == 0, torch.full_like(gt, 255), gt)
        gt_cls = torch.where(gt == 255, torch.zeros_like(gt), gt)
        max_regions = region_kwargs.get("max_regions", DEFAULT_MAX_REGIONS)
        truth = label_regions(gt_cls, None, connectivity=region_kwargs.get("connectivity", 8), min_area=gt_min_area,
                              max_regions=max_regions, scratch=self._scratch(RegionScratch, dev, H, W, max_regions))
        score = match_regions(out, truth, void=gt, void_value=255, iou_threshold=iou_threshold, max_pairs=max_pairs,
                              num_classes=self.num_classes, scratch=self._scratch(OverlapScratch, dev, max_pairs))
        if boundary_distance is not None:
            counts = boundary_counts(out["mask_clean"], gt, boundary_distance, self.num_classes, void_value=255,
                                     scratch=self._scratch(DistanceScratch, dev, 1, H, W))
            score["boundary"] = {"distance": int(boundary_distance), "counts": counts, **boundary_iou(counts)}
        out.update(score=score, gt_labels=truth["labels"], gt_regions=truth["regions"], gt_count=truth["count"])
        return out

    def detect_stack(self, scenes, *, valids=None, min_conf: float = 0.0, classes=1, words: Optional[int] = None, nodata=None,
                     min_valid: int = 1, fill: float = 0.0, norm=None, **follow_kwargs) -> dict:
        """One co-registered scene per date, oldest first: `predict` of each, its mask and confidence pushed into a
        `stack.DetectionStack` (`push(mask, conf=conf, min_conf=min_conf, classes=classes, valid=valids[i])`), then
        `stack.follow_sites(stack, **follow_kwargs)`: its result plus "stack". `valids`: None or one entry per scene, each None
        or a uint8 [H, W] map (numpy or tensor), 0 = not observed at that date. `words`: planes of 64 dates (None: as many as
        the scenes need). `nodata`, `min_valid`, `fill` and `norm` go to every date's `predict` (with `nodata`, next to `valids[i]`
        as its `valid`): the date's "valid" is what is pushed, so that a date's no-data is "not observed", not "observed, no
        hit", and neither breaks nor extends a run. Nothing scene-sized is kept per date beyond the stack's bits: a date's mask and confidence are
        released before the next scene is predicted."""
        from .stack import MAX_DATES, DetectionStack, follow_sites
        try:
            scenes = list(scenes)
        except TypeError:
            raise InsarError(f"detect_stack: scenes must be a sequence of 2-D scenes, got {type(scenes).__name__}") from None
        n = len(scenes)
        if not 1 <= n <= MAX_DATES:
            raise InsarError(f"detect_stack: {n} scenes: 1..{MAX_DATES}")
        shapes = {tuple(getattr(s, "shape", ())) for s in scenes}
        if len(shapes) != 1 or len(next(iter(shapes))) != 2:
            raise InsarError(f"detect_stack: the scenes must share one 2-D shape (co-register them first), got {sorted(shapes)}")
        H, W = next(iter(shapes))
        _check_geometry(H, W, self.tile, self.overlap)
        for s in scenes:                 # what `predict` would refuse, before the stack is allocated
            _check_validity("predict", H, W, getattr(s, "dtype", None) in (np.uint8, torch.uint8), self.tile, None, nodata, min_valid,
                            fill, norm)
        if valids is not None:
            valids = list(valids)
            if len(valids) != n:
                raise InsarError(f"detect_stack: {len(valids)} validity maps for {n} scenes")
        words = (n + 63) // 64 if words is None else words
        if isinstance(words, bool) or not isinstance(words, (int, np.integer)) or not (n + 63) // 64 <= words <= 4:
            raise InsarError(f"words={words!r}: an integer in {(n + 63) // 64}..4 for {n} scenes")
        try:
            device = next(self.model.parameters()).device
        except StopIteration:
            raise InsarError("ScenePredictor: the model has no parameters") from None
        st = DetectionStack(H, W, device, int(words))
        for i, scene in enumerate(scenes):
            v = None if valids is None else valids[i]
            if v is not None:
                v = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
                if not isinstance(v, torch.Tensor) or v.dtype != torch.uint8 or tuple(v.shape) != (H, W):
                    raise InsarError(f"detect_stack: valids[{i}] must be a uint8 [{H}, {W}] numpy array or tensor")
                v = v.detach().to(device).contiguous()
            out = self.predict(scene, nodata=nodata, min_valid=min_valid, fill=fill, norm=norm)
            if "valid" in out:
                v = out["valid"] if v is None else out["valid"] * (v != 0)
            st.push(out["mask"], conf=out["conf"], min_conf=min_conf, classes=classes, valid=v)
            del out
        res = follow_sites(st, **follow_kwargs)
        res["stack"] = st
        return res


def predict_scene(model: torch.nn.Module, scene, return_prob: bool = False, **kw) -> Dict[str, torch.Tensor]:
    """One-shot ScenePredictor(model, ...).predict(scene, return_prob, ...): `valid`, `nodata`, `min_valid`, `fill` and `norm`
    go to `predict`, every other keyword to the predictor."""
    run_kw = {k: kw.pop(k) for k in ("valid", "nodata", "min_valid", "fill", "norm") if k in kw}
    return ScenePredictor(model, **kw).predict(scene, return_prob=return_prob, **run_kw)


def detect_scene(model: torch.nn.Module, scene, return_prob: bool = False, **kw) -> dict:
    """One-shot ScenePredictor(model, ...).detect(scene, return_prob, ...): tile / overlap / batch / num_classes / tta go to
    the predictor, `outlines`, `simplify`, `skeletons`, `max_iterations`, `measure`, `split`, `sieve`, `hysteresis` and `contours` to
    `detect`, every other keyword to `label_regions`."""
    pred_kw = {k: kw.pop(k) for k in ("tile", "overlap", "batch", "num_classes", "tta") if k in kw}
    return ScenePredictor(model, **pred_kw).detect(scene, return_prob=return_prob, **kw)


def evaluate_scene(model: torch.nn.Module, scene, gt_mask, **kw) -> dict:
    """One-shot ScenePredictor(model, ...).evaluate(scene, gt_mask, ...): tile / overlap / batch / num_classes / tta go to the
    predictor, every other keyword to `evaluate`."""
    pred_kw = {k: kw.pop(k) for k in ("tile", "overlap", "batch", "num_classes", "tta") if k in kw}
    return ScenePredictor(model, **pred_kw).evaluate(scene, gt_mask, **kw)
