"""Exact Euclidean distance transform of a class or label map on the device (csrc/distance.hip: insar_dist_transform,
insar_dist_boundary_counts) and its three consumers: the void band round class borders, labels grown by a margin, and
boundary IoU.

Sites: ("eq", v) the pixels with m == v; ("ne", v) those with m != v; "edge" the pixels p with m[p] != ignore_value that have a
4-neighbour q inside the image with m[q] != ignore_value and m[q] != m[p] (both sides of a class border; the image border is
no border). `d2` is the squared distance to the nearest site of the same image in int32, exact, 0 on sites, FAR = 2^31 - 1
where it exceeds max_distance^2 or the image has no site; `nearest` the index y * W + x of a nearest site within its image
(-1 where d2 is FAR), of several the smallest. Integers only: every output is bitwise reproducible.

    out = distance_transform(mask, sites="edge", max_distance=32, ignore_value=255)       # two launches, no read-back
    train_mask = void_band(mask, 3)                                                       # 255 within 3 pixels of a border
    grown = expand_labels(det["labels"], 5)                                               # regions never merge
    counts = boundary_counts(pred_mask, gt_mask, 3, num_classes=2)                        # int64 [K, 3], one read-back
    boundary_iou(counts)["mean_iou"]
"""
from __future__ import annotations

from functools import partial
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_map, check_on_device, pinned, query_bytes, read_back

FAR = _lib.DIST_FAR
MAX_DIM = 32767
MAX_CLASSES = 8
_int = partial(check_int, integral_floats=True)      # this module's integers may come as floats with an integral value


def scratch_bytes(B: int, H: int, W: int) -> int:
    """Bytes of scratch of a B x H x W map. Host arithmetic only."""
    return query_bytes("insar_dist_scratch_bytes", B, H, W, outputs=1)


class DistanceScratch(Scratch):
    """The buffers of one (B, H, W): the column pass's result and, once `boundary_counts` has used it, the counts with the
    pinned host copy they are read back into. Nothing in them has to survive between calls."""
    KEY, SHOW, DEVICE_AT = ("B", "H", "W"), "{} x {} x {}", 3

    def __init__(self, B: int, H: int, W: int, device):
        super().__init__((B, H, W), device, scratch=scratch_bytes(B, H, W))
        self.counts = self.host = None

    def count_buffers(self):
        if self.counts is None:
            self.counts = torch.empty(MAX_CLASSES * 3, dtype=torch.int64, device=self.scratch.device)
            self.host = pinned(MAX_CLASSES * 3, torch.int64)
        return self.counts, self.host


def _map_dims(who: str, name: str, m, dtypes=(torch.uint8, torch.int32)):
    """(B, H, W) of a 2-D or 3-D map; everything but the device is checked here."""
    check_map(who, name, m, dtypes, dims=(2, 3), one_fault=True)
    B = 1 if m.dim() == 2 else m.shape[0]
    H, W = m.shape[-2], m.shape[-1]
    if B < 1 or H < 1 or W < 1 or H > MAX_DIM or W > MAX_DIM or B * H * W >= 1 << 31:
        raise InsarError(f"{who}: {name} {tuple(m.shape)}: need B, H, W >= 1, H, W <= {MAX_DIM} and B * H * W < 2^31")
    return int(B), int(H), int(W)


def _check_sites(who: str, sites, ignore_value):
    """(mode, value) of the C entry point."""
    if isinstance(sites, str) and sites == "edge":
        return _lib.DIST_EDGE, -1 if ignore_value is None else _int(who, "ignore_value", ignore_value, 0, (1 << 31) - 1)
    if isinstance(sites, (tuple, list)) and len(sites) == 2 and sites[0] in ("eq", "ne"):
        v = _int(who, f"sites[1] of {sites[0]!r}", sites[1], -(1 << 31), (1 << 31) - 1)
        return (_lib.DIST_EQ if sites[0] == "eq" else _lib.DIST_NE), v
    raise InsarError(f"{who}: sites={sites!r}: \"edge\", (\"eq\", v) or (\"ne\", v)")


def distance_transform(m: torch.Tensor, *, sites="edge", max_distance: Optional[int] = 32, ignore_value: Optional[int] = None,
                       return_nearest: bool = False, scratch: Optional[DistanceScratch] = None) -> dict:
    """The squared distance of every pixel of a device map (uint8 or int32, [H, W] or [B, H, W]) to the nearest site.

        out["d2"]       int32, the shape of m: 0 on sites, FAR where the distance exceeds max_distance or there is no site
        out["nearest"]  int32 (return_nearest=True): y * W + x of the nearest site within its image, -1 where d2 is FAR

    `max_distance`: a positive integer, or None for unbounded (the cost grows with the distances that occur).
    `ignore_value` belongs to sites="edge" alone. Two launches on the current stream; no read-back, no synchronisation.
    `scratch`: a DistanceScratch of this shape to reuse (else allocated)."""
    who = "distance_transform"
    B, H, W = _map_dims(who, "m", m)
    mode, value = _check_sites(who, sites, ignore_value)
    R = 0 if max_distance is None else _int(who, "max_distance", max_distance, 1, (1 << 31) - 1)
    if scratch is not None:
        DistanceScratch.check(who, scratch, (B, H, W), m.device)
    check_on_device(who, "m", m)
    if scratch is None:
        scratch = DistanceScratch(B, H, W, m.device)
    out = {"d2": torch.empty(m.shape, dtype=torch.int32, device=m.device)}
    if return_nearest:
        out["nearest"] = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        call("insar_dist_transform", ptr(m), _lib.DIST_U8 if m.dtype == torch.uint8 else _lib.DIST_I32, B, H, W, mode, value, R,
             ptr(scratch.scratch), ptr(out["d2"]), ptr(out.get("nearest")), _lib.stream_ptr())
    return out


def void_band(mask: torch.Tensor, width: int, *, void_value: int = 255, ignore_value: Optional[int] = 255) -> torch.Tensor:
    """uint8, the shape of `mask` ([H, W] or [B, H, W]): `void_value` wherever a class border lies within `width` pixels
    (d2 <= width^2 of the "edge" transform; width 0: the border pixels themselves), `mask` elsewhere. Pixels of
    `ignore_value` never make a border, and stay what they are."""
    who = "void_band"
    _map_dims(who, "mask", mask, dtypes=(torch.uint8,))
    width = _int(who, "width", width, 0, MAX_DIM)
    void_value = _int(who, "void_value", void_value, 0, 255)
    d2 = distance_transform(mask, sites="edge", max_distance=max(width, 1), ignore_value=ignore_value)["d2"]
    return torch.where(d2 <= width * width, torch.full_like(mask, void_value), mask)


def expand_labels(labels: torch.Tensor, distance: int) -> torch.Tensor:
    """int32, the shape of `labels` ([H, W] or [B, H, W]): every 0 pixel within `distance` of a labelled pixel takes the
    label of its nearest labelled pixel (of several, the one with the smallest index y * W + x); labelled pixels are
    unchanged, so regions never merge."""
    who = "expand_labels"
    B, H, W = _map_dims(who, "labels", labels, dtypes=(torch.int32,))
    distance = _int(who, "distance", distance, 0, MAX_DIM)
    out = distance_transform(labels, sites=("ne", 0), max_distance=max(distance, 1), return_nearest=True)
    near = out["nearest"].view(B, H * W)
    grown = torch.gather(labels.view(B, H * W), 1, near.clamp(min=0).long()).view(labels.shape)
    take = (labels == 0) & (out["d2"] <= distance * distance)
    return torch.where(take, grown, labels)


def _check_counts_args(who: str, pred, gt, distance, num_classes, void_value):
    B, H, W = _map_dims(who, "pred", pred, dtypes=(torch.uint8,))
    _map_dims(who, "gt", gt, dtypes=(torch.uint8,))
    if pred.dim() != 2 or tuple(gt.shape) != (H, W):
        raise InsarError(f"{who}: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must be 2-D maps of one shape")
    K = _int(who, "num_classes", num_classes, 2, MAX_CLASSES)
    d = _int(who, "distance", distance, 0, MAX_DIM)
    vv = -1 if void_value is None else _int(who, "void_value", void_value, 0, 255)
    return H, W, K, d, vv


def boundary_counts(pred: torch.Tensor, gt: torch.Tensor, distance: int, num_classes: int, *, void_value: Optional[int] = 255,
                    scratch: Optional[DistanceScratch] = None) -> np.ndarray:
    """int64 [K, 3] = (|P_c & G_c|, |P_c|, |G_c|) per class c of two device class maps uint8 [H, W], over the pixels with
    gt != void_value: P_c = the pixels of class c of `pred` within `distance` of a class border of `pred`, G_c the same of
    `gt`, whose void pixels make no border. Two transforms, a clear and the counts (six launches) on the current stream, and ONE
    read-back of 24 K bytes. `scratch`: a DistanceScratch(1, H, W) to reuse (else allocated)."""
    who = "boundary_counts"
    H, W, K, d, vv = _check_counts_args(who, pred, gt, distance, num_classes, void_value)
    if scratch is not None:
        DistanceScratch.check(who, scratch, (1, H, W), pred.device)
    check_on_device(who, "pred", pred)
    check_on_device(who, "gt", gt, like=pred)
    if scratch is None:
        scratch = DistanceScratch(1, H, W, pred.device)
    counts, host = scratch.count_buffers()
    d2p = distance_transform(pred, sites="edge", max_distance=max(d, 1), scratch=scratch)["d2"]
    d2g = distance_transform(gt, sites="edge", max_distance=max(d, 1), ignore_value=None if vv < 0 else vv, scratch=scratch)["d2"]
    with torch.cuda.device(pred.device):
        call("insar_dist_boundary_counts", ptr(pred), ptr(gt), ptr(d2p), ptr(d2g), H, W, d * d, K, vv, ptr(counts),
             _lib.stream_ptr())
        raw = read_back(host, counts)
    return raw[:3 * K].reshape(K, 3).copy()


def boundary_iou(counts) -> dict:
    """{"iou": float64 [K], inter / (p + g - inter) per class, NaN where the union is 0; "mean_iou": the mean over the
    foreground classes 1..K-1 whose union is not 0 (NaN if there is none)} of counts int64 [K, 3] as `boundary_counts` returns
    them. Counts of several scenes simply add. Pure numpy."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 2 or not np.issubdtype(c.dtype, np.integer) or (c < 0).any():
        raise InsarError(f"boundary_iou: counts must be a non-negative integer [K, 3] array with K >= 2, got {c.dtype} {c.shape}")
    c = c.astype(np.int64)
    union = c[:, 1] + c[:, 2] - c[:, 0]
    iou = np.full(c.shape[0], np.nan, dtype=np.float64)
    np.divide(c[:, 0].astype(np.float64), union.astype(np.float64), out=iou, where=union != 0)
    fg = union[1:] != 0
    return {"iou": iou, "mean_iou": float(np.mean(iou[1:][fg])) if fg.any() else float("nan")}
