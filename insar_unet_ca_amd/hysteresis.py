"""Hysteresis thresholds on the device (csrc/hysteresis.hip: insar_hyst_classify / _seeds / _keep / _apply around the
insar_regions_* phases): a site is a connected component of {score >= low} that holds at least one pixel with score >= high.
Extent comes from the permissive threshold, existence from the strict one, so the faint flanks of a real bowl stay with it and
a faint smear without a confident pixel is no site. `label_regions(min_conf=)` cuts pixel by pixel on the arg-max map;
`hysteresis_regions` works on the class scores themselves and can reach below the arg-max boundary.
`ScenePredictor.detect(..., hysteresis=(0.2, 0.8))` uses it in place of `label_regions`.

The rule (tests/hysteresis_ref.py restates it in numpy; DESIGN.md, "Hysteresis thresholds"): a pixel is a candidate of class c
if c is selected, score[c] >= low[c] in a float32 compare (NaN compares false) and the pixel is valid; of several classes the
greatest score wins, ties go to the smallest class; plane 0, the background, never takes part. `conf` is the winning class's
score, 0 where there is no candidate. A candidate is a seed if conf >= high[class]. Regions are the components of the candidate
map exactly as `label_regions` defines them; a region is kept if area >= min_area and it holds at least `min_seeds` seeds; the
kept regions are numbered 1..N in ascending root order. Everything behind the float32 compares is an integer: bitwise
reproducible.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_map, check_on_device, query_bytes, read_back
from .regions import DEFAULT_MAX_REGIONS, REGION_DTYPE, RegionScratch, regions_from_table
from .regions import _launch as _label_launch

LAUNCHES = 12                            # classify 1, the regions phases 7, seeds 2, keep 1, apply 1; ONE read-back
MAX_CLASSES = 256                        # the candidate map is uint8: classes 1..255 next to the background plane

# the C struct InsarHystRegion (include/insar_hip.h): an InsarRegion and the seed fields; record 0 is the header, whose `area`
# is the number of kept regions and whose `sum_y` the number of components of area >= min_area
HYST_DTYPE = np.dtype(REGION_DTYPE.descr + [("n_seed", "<i8"), ("peak_key", "<u8")])
assert HYST_DTYPE.itemsize == 80


def ordered_u32(x) -> np.ndarray:
    """The order-preserving map of float32 bits to uint32: all bits of a negative flipped, the sign bit of the rest. -0.0
    orders directly below 0.0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def from_ordered_u32(k) -> np.ndarray:
    """The float32 values of `ordered_u32` keys."""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def scratch_bytes(H: int, W: int, max_regions: int = DEFAULT_MAX_REGIONS):
    """(bytes of the seed table with the remap behind it, bytes of the compact table). Host arithmetic only."""
    return query_bytes("insar_hyst_scratch_bytes", H, W, max_regions, outputs=2)


class HysteresisScratch(Scratch):
    """The device buffers of one (H, W, max_regions): a RegionScratch for the labelling, the candidate map, the seed table with
    the remap, the threshold words, the compact table and the pinned host copy it is read back into. Nothing in them has to
    survive between calls."""
    KEY, SHOW, DEVICE_AT = ("H", "W", "max_regions"), "{} x {}, max_regions={}", 2

    def __init__(self, H: int, W: int, device: torch.device, max_regions: int = DEFAULT_MAX_REGIONS):
        sb, tb = scratch_bytes(H, W, max_regions)
        self.regions = RegionScratch(H, W, device, max_regions)
        super().__init__((H, W, max_regions), device, scratch=sb, table=tb, host=tb)
        self.cand = torch.empty(H, W, dtype=torch.uint8, device=device)
        self.thresholds = torch.empty(512, dtype=torch.float32, device=device)


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _per_class(who: str, name: str, v, K: int) -> np.ndarray:
    """float32 [K] indexed by class from a number (every class), a {class: number} dict (missing classes NaN) or a sequence
    of K numbers indexed by class (entry 0 is not looked at)."""
    out = np.full(K, np.nan, dtype=np.float32)
    if _is_number(v):
        out[:] = np.float32(v)
    elif isinstance(v, dict):
        for c, t in v.items():
            c = check_int(who, f"{name}: class", c, 1, K - 1, integral_floats=False)
            if not _is_number(t):
                raise InsarError(f"{who}: {name}[{c}]={t!r}: a finite number")
            out[c] = np.float32(t)
    elif isinstance(v, (list, tuple, np.ndarray)):
        if np.ndim(v) != 1 or len(v) != K:
            raise InsarError(f"{who}: {name}: a sequence indexed by class has {K} entries here, got shape {np.shape(v)}")
        for c, t in enumerate(v):
            t = t.item() if isinstance(t, np.generic) else t
            if not _is_number(t):
                raise InsarError(f"{who}: {name}[{c}]={t!r}: a finite number")
            out[c] = np.float32(t)
    else:
        raise InsarError(f"{who}: {name}={v!r}: a number, a {{class: number}} dict or a sequence indexed by class")
    return out


def threshold_words(low, high, classes, K: int, who: str = "hysteresis_regions") -> np.ndarray:
    """The 512 float32 words the kernels read: low[c] at word c, high[c] at word 256 + c for the selected classes, NaN (which
    no score reaches) everywhere else. `classes`: None (1..K-1) or a subset of it."""
    if classes is None:
        sel = list(range(1, K))
    else:
        try:
            sel = [check_int(who, "classes: class", c, 1, K - 1, integral_floats=False) for c in classes]
        except TypeError:
            raise InsarError(f"{who}: classes={classes!r}: None or a sequence of classes in 1..{K - 1}") from None
        if len(set(sel)) != len(sel):
            raise InsarError(f"{who}: classes={classes!r}: a class is named twice")
    lo, hi = _per_class(who, "low", low, K), _per_class(who, "high", high, K)
    words = np.full(512, np.nan, dtype=np.float32)
    for c in sel:
        if not np.isfinite(lo[c]):
            raise InsarError(f"{who}: low[{c}]={float(lo[c]):g}: a finite number")
        if not np.isfinite(hi[c]):
            raise InsarError(f"{who}: high[{c}]={float(hi[c]):g}: a finite number")
        if lo[c] > hi[c]:
            raise InsarError(f"{who}: low[{c}]={float(lo[c]):g} > high[{c}]={float(hi[c]):g}: low <= high")
        words[c], words[256 + c] = lo[c], hi[c]
    return words


def _check_args(score, low, high, classes, valid, connectivity, min_area, min_seeds, max_regions, scratch):
    """(H, W, K, words, min_area, min_seeds, max_regions): everything but the launches; the devices are looked at last."""
    who = "hysteresis_regions"
    check_map(who, "score", score, (torch.float32,), dims=(2, 3))
    H, W = (int(v) for v in score.shape[-2:])
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise InsarError(f"{who}: score {H} x {W}: need H, W >= 1 and H * W < 2^31")
    K = 2 if score.dim() == 2 else int(score.shape[0])
    if not 2 <= K <= MAX_CLASSES:
        raise InsarError(f"{who}: score {tuple(score.shape)}: a 3-D score needs the background plane 0 and 1..{MAX_CLASSES - 1} class "
                         f"planes behind it (a single class is a 2-D score)")
    words = threshold_words(low, high, classes, K, who)
    if valid is not None:
        check_map(who, "valid", valid, (torch.uint8,), shape=(H, W), of="score")
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise InsarError(f"{who}: connectivity={connectivity!r}: 4 or 8")
    min_area = check_int(who, "min_area", min_area, 1, integral_floats=True)
    min_seeds = check_int(who, "min_seeds", min_seeds, 1, integral_floats=True)
    max_regions = check_int(who, "max_regions", max_regions, 1, (1 << 31) - 2, integral_floats=True)
    if scratch is not None:
        HysteresisScratch.check(who, scratch, (H, W, max_regions), score.device)
    check_on_device(who, "score", score)
    if valid is not None:
        check_on_device(who, "valid", valid, like=score)
    return H, W, K, words, min_area, min_seeds, max_regions


def regions_from_hyst_table(raw: np.ndarray, W: int, max_regions: int) -> Dict[str, np.ndarray]:
    """The host table (fresh arrays) and the number of components that passed min_area, from the raw bytes of a compact
    table: raises if that number exceeds max_regions."""
    rec = raw.view(HYST_DTYPE)
    n, candidates = int(rec["area"][0]), int(rec["sum_y"][0])
    if candidates > max_regions:
        raise InsarError(f"hysteresis_regions: {candidates} regions of area >= min_area exceed max_regions={max_regions}: raise "
                         f"max_regions, min_area or low")
    rec = rec[:1 + n]
    plain = np.empty(1 + n, dtype=REGION_DTYPE)
    for f in REGION_DTYPE.names:
        plain[f] = rec[f]
    out = regions_from_table(plain.view(np.uint8), max_regions, True)
    key = rec["peak_key"][1:]
    index = np.uint32(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out["n_seed"] = rec["n_seed"][1:].astype(np.int64)
    out["peak"] = from_ordered_u32((key >> np.uint64(32)).astype(np.uint32))
    out["peak_y"], out["peak_x"] = (index // np.uint32(W)).astype(np.int32), (index % np.uint32(W)).astype(np.int32)
    return out, candidates


def hysteresis_regions(score: torch.Tensor, low, high, *, classes=None, valid: Optional[torch.Tensor] = None, connectivity: int = 8,
                       min_area: int = 1, min_seeds: int = 1, max_regions: int = DEFAULT_MAX_REGIONS,
                       scratch: Optional[HysteresisScratch] = None) -> dict:
    """Sites grown from confident seeds: the components of {score >= low} that hold a pixel with score >= high.

        out = hysteresis_regions(pred["prob"], 0.2, 0.8, min_area=20)
        out["labels"]  int32 [H, W]  0 or the region id 1..N     out["mask"]  uint8 [H, W]  the class at kept pixels, else 0
        out["conf"]    float32 [H, W]  the candidate plane: the winning class's score, 0 where there is no candidate
        out["count"]   N            out["candidates"]  components of area >= min_area before the seed rule
        out["regions"] dict of numpy arrays of length N: every field of `label_regions`' table over the whole low-threshold
        extent (mean_conf from `conf`), n_seed (int64), peak (float32, the exact maximum of conf), peak_y, peak_x (the first
        pixel in row-major order that reaches it)

    `score`: float32 [H, W] (one class, value 1) or [K, H, W] (class planes such as predict's "prob"; plane 0 is the background
    and is never a candidate, so a pixel with p(background) = 0.7 and p(site) = 0.3 is a candidate at low = 0.2). `low`, `high`:
    a number (every class), a {class: number} dict or a sequence of K numbers indexed by class; finite, low <= high. `classes`:
    a subset of 1..K-1 (None: all). `valid`: uint8 [H, W], 0 = never a candidate. With low == high the result is
    `label_regions(candidate map, conf, connectivity=, min_area=)`; raising `high` alone only removes regions. More than
    `max_regions` components of area >= min_area raise InsarError. 12 launches on the current stream and ONE device-to-host
    read-back (the compact table with its header). `scratch`: a HysteresisScratch of this scene size to reuse."""
    H, W, K, words, min_area, min_seeds, max_regions = _check_args(score, low, high, classes, valid, connectivity, min_area,
                                                                   min_seeds, max_regions, scratch)
    dev = score.device
    if scratch is None:
        scratch = HysteresisScratch(H, W, dev, max_regions)
    conf = torch.empty(H, W, dtype=torch.float32, device=dev)
    labels = torch.empty(H, W, dtype=torch.int32, device=dev)
    mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
    cand, thr, rs = scratch.cand, scratch.thresholds, scratch.regions
    planes = score.data_ptr() + (4 * H * W if score.dim() == 3 else 0)          # the background plane is not passed
    with torch.cuda.device(dev):
        s = _lib.stream_ptr()
        thr.copy_(torch.from_numpy(words), non_blocking=False)
        call("insar_hyst_classify", planes, K - 1, H, W, ptr(thr), ptr(valid), ptr(cand), ptr(conf), s)
        # the labelling of regions.py over the candidate map; min_conf = -inf: it drops nothing
        _label_launch(cand, conf, int(connectivity), min_area, float("-inf"), max_regions, rs.scratch, rs.table, labels, mask)
        call("insar_hyst_seeds", ptr(labels), ptr(cand), ptr(conf), ptr(thr), H, W, max_regions, ptr(scratch.scratch), s)
        call("insar_hyst_keep", ptr(rs.table), min_seeds, max_regions, ptr(scratch.scratch), ptr(scratch.table), s)
        call("insar_hyst_apply", ptr(cand), H, W, max_regions, ptr(scratch.scratch), ptr(labels), ptr(mask), s)
        raw = read_back(scratch.host, scratch.table)
    regions, candidates = regions_from_hyst_table(raw, W, max_regions)
    return {"labels": labels, "mask": mask, "conf": conf, "count": int(len(regions["id"])), "regions": regions,
            "candidates": candidates}


__all__ = ["HYST_DTYPE", "HysteresisScratch", "hysteresis_regions", "ordered_u32", "scratch_bytes", "threshold_words"]
