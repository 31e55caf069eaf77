"""Training from whole scenes (csrc/crops.hip): the training-side mirror of `infer.ScenePredictor`. A scene and its label map
stay resident on the device and every batch is cut from them at origins drawn on the device, balanced over classes by a
per-class summed-area table of the labels (`CropIndex`) and kept away from void regions.

The draw is a pure function of (seed, rank, step): two runs, or a run resumed from `state_dict()`, see the same stream of
crops, and nothing is read back from the device per batch (the only read-back is one `class_pixels()` per scene when a
`SceneCrops` is built). Per batch: insar_crops_draw, insar_crops_gather, and the two launches of `Augment` if one is given;
with a `WarpSpec` (warp.py) insar_crops_draw, insar_warp_draw, insar_warp_gather: one launch more, still nothing read back.

The draw rule (include/insar_hip.h: insar_crops_draw; tests/crops_ref.py restates it): with h(i) = aug_hash64(key, i), sample s
uses the counter base b = 65 s; its target class is the first c with float32(h(b) >> 40) * 2^-24 < cum[c]; try t < tries has
the origin (cy g, cx g) with r = h(b + 1 + t), cy = ((r >> 32) ny) >> 32, cx = ((r & 0xffffffff) nx) >> 32; the lowest try
whose tile holds >= min_count target pixels and <= max_void void pixels wins; if there is none, the try with the most target
pixels among those within the void cap, and if none is within it the try with the fewest void pixels (ties to the lowest t).
"""
from __future__ import annotations

import ctypes as C
import math
from functools import partial
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import check_int
from .augment import MASK64, Augment, aug_hash64
from .infer import MAX_CLASSES, _as_scene
from .warp import WarpSpec, draw_warps, gather_warped

CROP_STREAM = 0xDA942042E4DD58B5           # separates the crop keys from the augmentation table's and the noise seeds' (NOISE_STREAM)
SCENE_STREAM = 0x2545F4914F6CDD1D          # the second hash of a batch key, which picks the scene
MAX_TRIES = 64
_MASK_CODES = {torch.uint8: _lib.AUG_MASK_U8, torch.int64: _lib.AUG_MASK_I64}


_int = partial(check_int, None, integral_floats=False)        # the strict rule, the argument named without a tool


def _check_classes(K) -> int:
    K = _int("num_classes", K, 0)
    if not 2 <= K <= MAX_CLASSES:
        raise InsarError(f"num_classes={K}: the crop kernels cover 2..{MAX_CLASSES} classes")
    return K


def check_geometry(H: int, W: int, tile: int, cell: int) -> None:
    """What the kernels ask of a scene, a tile and a cell size (host arithmetic; the entry points check the same)."""
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise InsarError(f"scene {H} x {W}: at least one pixel and fewer than 2^31")
    if cell < 1 or cell > min(H, W):
        raise InsarError(f"cell={cell}: must lie in 1..min(H, W) = {min(H, W)}")
    if tile < 4 or tile % 4 or tile % cell:
        raise InsarError(f"tile={tile}: must be a positive multiple of 4 and of the cell size {cell}")
    if tile > H or tile > W:
        raise InsarError(f"scene {H} x {W} is smaller than the tile {tile}: there is no padding path")


def batch_key(seed: int, rank: int, step: int) -> int:
    """The key of batch `step`: aug_hash64(aug_hash64(seed, rank) ^ CROP_STREAM, step)."""
    return aug_hash64(aug_hash64(int(seed) & MASK64, int(rank)) ^ CROP_STREAM, int(step) & MASK64)


def pick_scene(key: int, candidates: Sequence[int]) -> int:
    """The scene of the batch with key `key`: index i with probability candidates[i] / sum(candidates) (the numbers of
    candidate origins), by a multiply-shift of a second hash of the key. Host integers only."""
    total = sum(candidates)
    if total < 1 or any(c < 0 for c in candidates):
        raise InsarError(f"pick_scene: candidate counts {list(candidates)}")
    v = (aug_hash64(key ^ SCENE_STREAM, 0) * total) >> 64
    acc = 0
    for i, c in enumerate(candidates):
        acc += c
        if v < acc:
            return i
    return len(candidates) - 1


def count_limits(tile: int, min_fraction: float, max_void_fraction: float):
    """(min_count, max_void) = (ceil(min_fraction tile^2), floor(max_void_fraction tile^2))."""
    for name, f in (("min_fraction", min_fraction), ("max_void_fraction", max_void_fraction)):
        if isinstance(f, bool) or not isinstance(f, (int, float, np.floating, np.integer)) or not 0.0 <= float(f) <= 1.0:
            raise InsarError(f"{name}={f!r}: a number in 0..1")
    area = tile * tile
    return int(math.ceil(float(min_fraction) * area)), int(math.floor(float(max_void_fraction) * area))


def cumulative(probs: Sequence[float]) -> np.ndarray:
    """float32 [K]: the running float32 sums of probs / sum(probs), the last one forced to 1 (the table the draw compares with)."""
    p = np.asarray(list(probs), dtype=np.float64)
    if p.ndim != 1 or p.size < 1 or not np.isfinite(p).all() or (p < 0).any() or p.sum() <= 0:
        raise InsarError(f"class_probs={list(probs)!r}: non-negative numbers with a positive sum")
    cum = np.cumsum((p / p.sum()).astype(np.float32), dtype=np.float32)
    cum[-1] = np.float32(1.0)
    return cum


def make_state(seed: int, rank: int, step: int, config: dict) -> dict:
    return {"seed": int(seed), "rank": int(rank), "step": int(step), "config": dict(config)}


def check_state(state: dict):
    """-> (seed, rank, step, config) of a `state_dict()`, or InsarError."""
    try:
        seed, rank, step, cfg = int(state["seed"]), int(state["rank"]), int(state["step"]), dict(state["config"])
    except (KeyError, TypeError, ValueError) as e:
        raise InsarError(f"SceneCrops.load_state_dict: malformed state ({e!r})") from None
    if seed < 0 or rank < 0 or step < 0:
        raise InsarError(f"SceneCrops.load_state_dict: seed={seed}, rank={rank}, step={step}")
    return seed & MASK64, rank, step, cfg


def _as_labels(labels, device: torch.device) -> torch.Tensor:
    dt = getattr(labels, "dtype", None)
    if dt not in (np.uint8, torch.uint8):
        raise InsarError(f"labels dtype {dt}: uint8 (255 = void)")
    return _as_scene(labels, device)


class CropIndex:
    """The per-class summed-area table of a label map: int32 [K + 1, Hc + 1, Wc + 1] with Hc = H // cell, Wc = W // cell.

        idx = CropIndex(labels, num_classes=2, cell=8)      # labels: uint8 [H, W], numpy or torch, host or device
        idx.table[p, a, b]     pixels with label p (p = K: void, i.e. 255 and every label >= K) in rows < a * cell, columns < b * cell
        idx.counts(origins, tile)    int32 [n, K + 1] on the device       idx.class_pixels()    int64 [K] on the device

    Built once, on the current stream (insar_crops_cells, insar_crops_sat: 3 launches); nothing is read back."""

    def __init__(self, labels, num_classes: int, cell: int = 8, device=None):
        self.num_classes = _check_classes(num_classes)
        self.cell = _int("cell", cell, 1)
        if device is None:
            device = labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else torch.device("cuda")
        self.labels = _as_labels(labels, torch.device(device))
        self.H, self.W = (int(v) for v in self.labels.shape)
        if self.H * self.W >= 1 << 31 or self.cell > min(self.H, self.W):
            raise InsarError(f"labels {self.H} x {self.W}, cell {self.cell}: fewer than 2^31 pixels and cell <= min(H, W)")
        self.Hc, self.Wc = self.H // self.cell, self.W // self.cell
        dev = self.labels.device
        with torch.cuda.device(dev):
            self.table = torch.empty(self.num_classes + 1, self.Hc + 1, self.Wc + 1, dtype=torch.int32, device=dev)
            call("insar_crops_cells", ptr(self.labels), self.H, self.W, self.num_classes, self.cell, ptr(self.table), _lib.stream_ptr())
            call("insar_crops_sat", ptr(self.table), self.num_classes, self.Hc, self.Wc, _lib.stream_ptr())

    @property
    def nbytes(self) -> int:
        return self.table.numel() * 4

    def candidates(self, tile: int) -> int:
        """The number of origins a draw can produce for `tile`: (Hc - tile / cell + 1) * (Wc - tile / cell + 1)."""
        check_geometry(self.H, self.W, tile, self.cell)
        return (self.Hc - tile // self.cell + 1) * (self.Wc - tile // self.cell + 1)

    def counts(self, origins: torch.Tensor, tile: int) -> torch.Tensor:
        """int32 [n, K + 1]: the pixels per class (last column: void) of the tile x tile crops at `origins` (device integer
        [n, 2], multiples of the cell size), by plain torch indexing of the table; stays on the device."""
        check_geometry(self.H, self.W, tile, self.cell)
        if not isinstance(origins, torch.Tensor) or origins.dim() != 2 or origins.shape[1] != 2 or origins.device != self.table.device:
            raise InsarError("CropIndex.counts: origins must be an integer [n, 2] tensor on the table's device")
        o = origins.long()
        a0, b0 = o[:, 0] // self.cell, o[:, 1] // self.cell
        a1, b1 = a0 + tile // self.cell, b0 + tile // self.cell
        t = self.table
        return (t[:, a1, b1] - t[:, a0, b1] - t[:, a1, b0] + t[:, a0, b0]).t().contiguous()

    def class_pixels(self) -> torch.Tensor:
        """int64 [K] on the device: the pixels per class inside the cells (the ragged far edges excluded), as `class_weights`
        takes them after a `.cpu()`."""
        return self.table[:self.num_classes, self.Hc, self.Wc].long()


def draw_crops(index: CropIndex, key: int, n: int, tile: int, cum: np.ndarray, min_count: int, max_void: int, tries: int):
    """insar_crops_draw on the current stream -> (origins int32 [n, 2], info int32 [n, 4]), fresh device tensors."""
    dev = index.table.device
    cum = np.ascontiguousarray(cum, dtype=np.float32)
    if cum.shape != (index.num_classes,):
        raise InsarError(f"draw_crops: cum {cum.shape}: one float32 per class ({index.num_classes})")
    origins = torch.empty(int(n), 2, dtype=torch.int32, device=dev)
    info = torch.empty(int(n), 4, dtype=torch.int32, device=dev)
    call("insar_crops_draw", int(key) & MASK64, int(n), index.num_classes, int(tries), cum.ctypes.data_as(C.c_void_p), int(min_count),
         int(max_void), int(tile), index.cell, index.H, index.W, ptr(index.table), ptr(origins), ptr(info), _lib.stream_ptr())
    return origins, info


def gather_crops(scene: Optional[torch.Tensor], labels: Optional[torch.Tensor], origins: torch.Tensor, tile: int,
                 mask_dtype: torch.dtype = torch.int64):
    """insar_crops_gather on the current stream -> (images float32 [n, 1, tile, tile] or None, masks [n, tile, tile] or None)
    from a device scene (uint8 / float32 [H, W]) and / or a device label map (uint8 [H, W]) at the device table `origins`."""
    ref = scene if scene is not None else labels
    if ref is None:
        raise InsarError("gather_crops: neither a scene nor labels")
    for name, t, dts in (("scene", scene, (torch.uint8, torch.float32)), ("labels", labels, (torch.uint8,))):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or t.dtype not in dts or not t.is_contiguous():
            raise InsarError(f"gather_crops: {name} must be a contiguous 2-D ROCm tensor of dtype {' or '.join(str(d) for d in dts)}")
        if t.shape != ref.shape or t.device != ref.device:
            raise InsarError("gather_crops: scene and labels must have one shape and lie on one device")
    if mask_dtype not in _MASK_CODES:
        raise InsarError(f"gather_crops: mask_dtype {mask_dtype}: torch.int64 or torch.uint8")
    if (not isinstance(origins, torch.Tensor) or origins.device != ref.device or origins.dtype != torch.int32 or origins.dim() != 2
            or origins.shape[1] != 2 or not origins.is_contiguous()):
        raise InsarError("gather_crops: origins must be a contiguous int32 [n, 2] tensor on the scene's device")
    n, (H, W) = origins.shape[0], ref.shape
    images = torch.empty(n, 1, tile, tile, dtype=torch.float32, device=ref.device) if scene is not None else None
    masks = torch.empty(n, tile, tile, dtype=mask_dtype, device=ref.device) if labels is not None else None
    code = _lib.SCENE_F32 if scene is not None and scene.dtype == torch.float32 else _lib.SCENE_U8
    call("insar_crops_gather", ptr(scene), code, ptr(labels), H, W, ptr(origins), n, int(tile), ptr(images), ptr(masks),
         _MASK_CODES[mask_dtype], _lib.stream_ptr())
    return images, masks


class SceneCrops:
    """A training loader that cuts class-balanced crops from resident scenes on the device.

        crops = SceneCrops(scene, labels, tile=256, batch=16, steps_per_epoch=200, num_classes=2, seed=0, rank=rank,
                           augment=Augment(seed=0, rank=rank))
        for images, masks in crops: ...            # float32 [batch, 1, tile, tile], int64 [batch, tile, tile], device tensors
        train_model(net, crops, val_loader, criterion, optimizer, device)

    `scenes` / `labels`: one scene (2-D uint8 or float32, numpy or torch, as `ScenePredictor` takes it) and its uint8 label map
    (255 = void), or equal-length lists; with several scenes each batch comes from one of them, chosen on the host with
    probability proportional to its number of candidate origins. `class_probs` (None: uniform over the classes present in
    the scenes) gives the target-class distribution; a crop is accepted with >= ceil(min_fraction tile^2) pixels of its
    target class and <= floor(max_void_fraction tile^2) void pixels, after at most `tries` (1..64) tries, else the best try
    is taken (module docstring). `last_info` is the device table int32 [batch, 4] of the last batch: target class, accepted
    try or -1, target pixels, void pixels. `state_dict()` / `load_state_dict()` carry {seed, rank, step, config}.

    `warp`: a `WarpSpec` rotates and zooms every crop about the centre of its drawn tile (bilinear image, nearest labels;
    what leaves the scene is 0 in the image and void in the mask); `last_matrices` then holds the batch's Q32 warps, int64
    [batch, 6]. None is the axis-aligned path, launch for launch. Known limit: the class-balance test of the draw and the
    counts in `last_info` refer to the axis-aligned tile at the drawn origin, not to the warped footprint."""

    def __init__(self, scenes, labels, tile: int = 256, batch: int = 16, steps_per_epoch: int = 100, num_classes: int = 2,
                 class_probs: Optional[Sequence[float]] = None, min_fraction: float = 0.01, max_void_fraction: float = 0.5,
                 tries: int = 16, cell: int = 8, seed: int = 0, rank: int = 0, augment: Optional[Augment] = None,
                 mask_dtype: torch.dtype = torch.int64, device=None, warp: Optional[WarpSpec] = None):
        self.num_classes = _check_classes(num_classes)
        self.tile, self.batch = _int("tile", tile, 1), _int("batch", batch, 1)
        self.steps_per_epoch, self.cell = _int("steps_per_epoch", steps_per_epoch, 1), _int("cell", cell, 1)
        self.tries = _int("tries", tries, 1)
        if self.tries > MAX_TRIES:
            raise InsarError(f"tries={tries}: at most {MAX_TRIES} (one lane of a wave per try)")
        self.seed, self.rank, self.step = _int("seed", seed, 0) & MASK64, _int("rank", rank, 0), 0
        if mask_dtype not in _MASK_CODES:
            raise InsarError(f"mask_dtype {mask_dtype}: torch.int64 or torch.uint8")
        if augment is not None and not isinstance(augment, Augment):
            raise InsarError("augment must be an Augment")
        if augment is not None and mask_dtype != torch.int64:
            raise InsarError("augment returns int64 masks: mask_dtype must be torch.int64 with it")
        if warp is not None and not isinstance(warp, WarpSpec):
            raise InsarError("warp must be a WarpSpec")
        self.mask_dtype, self.augment, self.warp = mask_dtype, augment, warp
        self.min_fraction, self.max_void_fraction = float(min_fraction), float(max_void_fraction)
        self.min_count, self.max_void = count_limits(self.tile, min_fraction, max_void_fraction)
        if isinstance(scenes, (list, tuple)) != isinstance(labels, (list, tuple)):
            raise InsarError("scenes and labels: a single scene with its label map, or two lists")
        scenes, labels = (list(scenes), list(labels)) if isinstance(scenes, (list, tuple)) else ([scenes], [labels])
        if len(scenes) != len(labels) or not scenes:
            raise InsarError(f"{len(scenes)} scenes, {len(labels)} label maps")
        for sc, lb in zip(scenes, labels):
            hs, hl = tuple(getattr(sc, "shape", ())), tuple(getattr(lb, "shape", ()))
            if len(hs) != 2 or hs != hl:
                raise InsarError(f"scene {hs} and its label map {hl}: two 2-D arrays of one shape")
            check_geometry(hs[0], hs[1], self.tile, self.cell)                 # refuse before anything is copied
        dev = torch.device("cuda" if device is None else device)
        self.scenes: List[torch.Tensor] = [_as_scene(sc, dev) for sc in scenes]
        self.indices: List[CropIndex] = [CropIndex(lb, self.num_classes, self.cell, device=dev) for lb in labels]
        self.candidates = [ix.candidates(self.tile) for ix in self.indices]
        if class_probs is None:
            pixels = torch.stack([ix.class_pixels() for ix in self.indices]).sum(0).cpu().tolist()      # the one read-back
            if not any(pixels):
                raise InsarError("the scenes hold no pixel of any class (all void): give class_probs")
            class_probs = [1.0 if v > 0 else 0.0 for v in pixels]
        if len(list(class_probs)) != self.num_classes:
            raise InsarError(f"class_probs: {self.num_classes} numbers, one per class")
        self.class_probs = [float(v) for v in class_probs]
        self.cum = cumulative(self.class_probs)
        self.last_info: Optional[torch.Tensor] = None
        self.last_origins: Optional[torch.Tensor] = None
        self.last_matrices: Optional[torch.Tensor] = None
        self.last_scene: Optional[int] = None

    def __len__(self) -> int:
        return self.steps_per_epoch

    def _config(self) -> dict:
        cfg = {"tile": self.tile, "batch": self.batch, "num_classes": self.num_classes, "class_probs": list(self.class_probs),
               "min_fraction": self.min_fraction, "max_void_fraction": self.max_void_fraction, "tries": self.tries,
               "cell": self.cell, "scene_shapes": [[ix.H, ix.W] for ix in self.indices]}
        if self.warp is not None:
            cfg["warp"] = self.warp.config()
        return cfg

    def state_dict(self) -> dict:
        state = make_state(self.seed, self.rank, self.step, self._config())
        if self.augment is not None:
            state["augment"] = self.augment.state_dict()
        return state

    def load_state_dict(self, state: dict) -> None:
        seed, rank, step, cfg = check_state(state)
        if cfg != self._config():
            raise InsarError(f"SceneCrops.load_state_dict: the state's config {cfg} is not this object's {self._config()}: "
                             "the stream would not continue")
        self.seed, self.rank, self.step = seed, rank, step
        if self.augment is not None and "augment" in state:
            self.augment.load_state_dict(state["augment"])

    def key(self, step: Optional[int] = None) -> int:
        return batch_key(self.seed, self.rank, self.step if step is None else step)

    def next_batch(self):
        """The batch of the current step (which it advances): (images, masks), fresh device tensors on the current stream."""
        key = self.key()
        i = pick_scene(key, self.candidates)
        index, scene = self.indices[i], self.scenes[i]
        with torch.cuda.device(scene.device):
            origins, info = draw_crops(index, key, self.batch, self.tile, self.cum, self.min_count, self.max_void, self.tries)
            if self.warp is None:
                matrices = None
                images, masks = gather_crops(scene, index.labels, origins, self.tile, self.mask_dtype)
            else:
                matrices = draw_warps(key, origins, self.tile, self.warp)
                images, masks = gather_warped(scene, index.labels, matrices, self.tile, self.mask_dtype)
        self.last_info, self.last_origins, self.last_scene, self.last_matrices = info, origins, i, matrices
        self.step += 1
        if self.augment is not None:
            images, masks = self.augment(images, masks)
        return images, masks

    def __iter__(self):
        for _ in range(self.steps_per_epoch):
            yield self.next_batch()
