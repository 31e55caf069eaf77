"""Splitting touching sites: a watershed of a height map inside every region of a label map, on the device (csrc/split.hip:
insar_split_basins / _rounds / _finish). `label_regions` knows a site only as a connected component, so two subsidence bowls
whose masks touch are one region; `split_regions` cuts such a region along the necks of its distance map and hands back a label
map and table of exactly the shape `label_regions` returns, so outlines, centre lines, zonal statistics and scoring work on the
pieces unchanged. `ScenePredictor.detect(..., split=1.0)` splits what it labelled.

The rule, in integers (tests/split_ref.py restates it in numpy; DESIGN.md, "Splitting touching sites"): with
key(p) = (h[p], -index(p)), every foreground pixel points to the greatest-key pixel among itself and its 8 neighbours of the same
label; pixels that point to themselves are the roots of the basins. saddle(a, b) of two basins of one label is the maximum of
min(h[p], h[q]) over 8-adjacent p in a, q in b. Pieces start as the basins and merge in synchronous rounds: every piece u finds
the neighbouring piece v with the greatest (saddle(u, v), key(root v)) and merges into it iff depth(h[root u], saddle) <= T and
key(root v) > key(root u); pointers are compressed and the next round sees the merged pieces. Squared heights measure depth in
sixteenths of a pixel, depth(P, S) = isqrt(256 P) - isqrt(256 S) and T = rint(16 min_depth); linear heights (`squared=False`)
as P - S and T = min_depth. At the fixed point no piece has a neighbour whose saddle lies within `min_depth` of its peak.
Pieces are numbered 1..M by ascending smallest row-major pixel index, which is `label_regions`'s order: a label map that no cut
touches comes back with the same partition and numbering.

By default h is distance_transform(labels, sites="edge", max_distance=max_distance)["d2"], far values taken as max_distance^2.
Under the "edge" sites the image border is no border: a bowl cut by the scene edge keeps rising towards it, so its summit lies on
the scene edge, and a label that fills the whole map is one plateau and comes back whole.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import MERGE_CTRL_WORDS as CTRL_WORDS  # noqa: F401  pairs, overflow, negative heights, basins, pieces, 3 spare
from ._scene import MERGE_ROUNDS_PER_READ as ROUNDS_PER_READ  # noqa: F401  (the tools read them from here)
from ._scene import Scratch, check_int, check_map, check_on_device, merge_rounds, pinned, query_bytes, read_back
from .distance import MAX_DIM, DistanceScratch, distance_transform
from .regions import CONF_SCALE, DEFAULT_MAX_REGIONS

DEFAULT_MAX_PAIRS = 1 << 20
MAX_PAIRS = 1 << 24
MAX_ROUNDS = 4096
MAX_THRESHOLD = 1 << 20

# the C struct InsarSplitRegion (include/insar_hip.h); record 0 of a table is the header
SPLIT_DTYPE = np.dtype([("area", "<i8"), ("sum_y", "<i8"), ("sum_x", "<i8"), ("sum_conf", "<i8"),
                        ("y0", "<i4"), ("x0", "<i4"), ("y1", "<i4"), ("x1", "<i4"),
                        ("first", "<i4"), ("cls", "<i4"), ("parent", "<i4"), ("peak", "<i4"),
                        ("peak_index", "<i4"), ("saddle", "<i4"), ("_pad", "<i4", (2,))])
assert SPLIT_DTYPE.itemsize == 80


def scratch_bytes(H: int, W: int, max_regions: int = DEFAULT_MAX_REGIONS, max_pairs: int = DEFAULT_MAX_PAIRS,
                  max_rounds: int = 64):
    """(scratch bytes, table bytes, offset of the control words in the scratch, their bytes). Host arithmetic only."""
    return query_bytes("insar_split_scratch_bytes", H, W, max_regions, max_pairs, max_rounds, outputs=4)


class SplitScratch(Scratch):
    """The device buffers of one (H, W, max_regions, max_pairs, max_rounds): scratch, the piece table, and the pinned host
    copies of the table and the control words. Nothing in them has to survive between calls."""
    KEY, DEVICE_AT = ("H", "W", "max_regions", "max_pairs", "max_rounds"), 2

    def __init__(self, H: int, W: int, device, max_regions: int = DEFAULT_MAX_REGIONS, max_pairs: int = DEFAULT_MAX_PAIRS,
                 max_rounds: int = 64):
        sb, tb, off, cb = scratch_bytes(H, W, max_regions, max_pairs, max_rounds)
        super().__init__((H, W, max_regions, max_pairs, max_rounds), device, scratch=sb, table=tb, host=tb)
        self.ctrl, self.ctrl_host = self.scratch[off:off + cb], pinned(cb)
        self.distance = None                                      # DistanceScratch of the default height map, made on first use


def _threshold(who: str, min_depth, squared: bool) -> int:
    ok = isinstance(min_depth, (int, float, np.integer, np.floating)) and not isinstance(min_depth, bool) and np.isfinite(min_depth)
    if ok and not squared:
        ok = int(min_depth) == min_depth
    T = int(np.rint(float(min_depth) * 16.0)) if ok and squared else int(min_depth) if ok else -1
    if not ok or T < 0 or T > MAX_THRESHOLD:
        unit = "a number with 0 <= 16 * min_depth <= 2^20 (pixels)" if squared else "an integer in 0..2^20 (height units)"
        raise InsarError(f"{who}: min_depth={min_depth!r}: {unit}")
    return T


def _check_args(labels, mask, conf, height, squared, min_depth, max_distance, max_regions, max_pairs, max_rounds, scratch):
    """(H, W, squared, T, R): everything but the launches; the devices are looked at last."""
    who = "split_regions"
    check_map(who, "labels", labels, (torch.int32,))
    H, W = labels.shape
    if H < 1 or W < 1 or H > MAX_DIM or W > MAX_DIM or H * W >= 1 << 31:
        raise InsarError(f"{who}: labels {H} x {W}: need 1 <= H, W <= {MAX_DIM} and H * W < 2^31")
    if mask is not None:
        check_map(who, "mask", mask, (torch.uint8,), shape=(H, W))
    if conf is not None:
        check_map(who, "conf", conf, (torch.float32,), shape=(H, W))
    if height is not None:
        check_map(who, "height", height, (torch.int32,), shape=(H, W))
        if max_distance is not None:
            raise InsarError(f"{who}: max_distance belongs to the default height map, not to height=")
    if squared is None:
        squared = height is None
    if not isinstance(squared, (bool, np.bool_)):
        raise InsarError(f"{who}: squared={squared!r}: True, False or None")
    T = _threshold(who, min_depth, bool(squared))
    R = 0 if max_distance is None else check_int(who, "max_distance", max_distance, 1, MAX_DIM, integral_floats=True)
    caps = (check_int(who, "max_regions", max_regions, 1, (1 << 31) - 2, integral_floats=True),
            check_int(who, "max_pairs", max_pairs, 1, MAX_PAIRS, integral_floats=True),
            check_int(who, "max_rounds", max_rounds, 1, MAX_ROUNDS, integral_floats=True))
    if scratch is not None:
        SplitScratch.check(who, scratch, (H, W) + caps, labels.device)
    check_on_device(who, "labels", labels)
    for name, t in (("mask", mask), ("conf", conf), ("height", height)):
        if t is not None:
            check_on_device(who, name, t, like=labels)
    return int(H), int(W), bool(squared), T, R


def pieces_from_table(raw: np.ndarray, W: int, max_regions: int, with_conf: bool) -> Dict[str, np.ndarray]:
    """The host table (fresh arrays) from the raw bytes of a device table: the fields of `regions_from_table` plus parent,
    peak, peak_y, peak_x and saddle. Raises if the count in the header exceeds max_regions."""
    rec = raw.view(SPLIT_DTYPE)
    n = int(rec["area"][0])
    if n > max_regions:
        raise InsarError(f"split_regions: {n} pieces exceed max_regions={max_regions}: raise max_regions or min_depth")
    r = rec[1:1 + n]
    area = r["area"].astype(np.int64)
    out = {"id": np.arange(1, n + 1, dtype=np.int32), "cls": r["cls"].astype(np.int32), "area": area,
           "y0": r["y0"].copy(), "x0": r["x0"].copy(), "y1": r["y1"].copy(), "x1": r["x1"].copy(),
           "cy": r["sum_y"].astype(np.float64) / area, "cx": r["sum_x"].astype(np.float64) / area}
    if with_conf:
        out["mean_conf"] = r["sum_conf"].astype(np.float64) / (area.astype(np.float64) * CONF_SCALE)
    out.update(parent=r["parent"].copy(), peak=r["peak"].copy(), peak_y=(r["peak_index"] // W).astype(np.int32),
               peak_x=(r["peak_index"] % W).astype(np.int32), saddle=r["saddle"].copy())
    return out


def split_regions(labels: torch.Tensor, *, mask: Optional[torch.Tensor] = None, conf: Optional[torch.Tensor] = None,
                  height: Optional[torch.Tensor] = None, squared: Optional[bool] = None, min_depth: float = 1.0,
                  max_distance: Optional[int] = None, max_regions: int = DEFAULT_MAX_REGIONS, max_pairs: int = DEFAULT_MAX_PAIRS,
                  max_rounds: int = 64, scratch: Optional[SplitScratch] = None) -> dict:
    """The regions of a device label map (int32 [H, W]; <= 0 background, any positive ids) cut along the necks of a height map.

        out = split_regions(det["labels"], mask=det["mask_clean"], conf=det["conf"], min_depth=1.0)
        out["labels"]   int32 [H, W]  0 or the piece id 1..M      out["count"]  M
        out["regions"]  dict of numpy arrays of length M: the fields of label_regions (id, cls from `mask` else 0, area, y0, x0,
                        y1, x1, cy, cx[, mean_conf with `conf`]) plus parent (the input label), peak (the height at the piece's
                        root), peak_y, peak_x and saddle (the greatest saddle towards a neighbouring piece, -1 if none)
        out["raw_basins"]  basins before merging     out["rounds"]  rounds that merged something
        out["converged"]   whether a round that merged nothing was reached within `max_rounds` rounds

    `height`: int32 [H, W] >= 0 of your own (then `squared` defaults to False: depths are plain differences and `min_depth`
    an integer); by default the squared distance to the region border (`squared` True: `min_depth` in pixels, to 1/16),
    unbounded or clamped at `max_distance`. More than `max_pairs` adjacent basin pairs, or more than `max_regions` pieces, raise
    InsarError. 11 launches plus 4 per round on the current stream (2 more for the default height map); the host reads the
    control words once per 4 rounds and the table once. `scratch`: a SplitScratch of this shape to reuse (else allocated)."""
    who = "split_regions"
    H, W, squared, T, R = _check_args(labels, mask, conf, height, squared, min_depth, max_distance, max_regions, max_pairs,
                                      max_rounds, scratch)
    max_regions, max_pairs, max_rounds = int(max_regions), int(max_pairs), int(max_rounds)
    if scratch is None:
        scratch = SplitScratch(H, W, labels.device, max_regions, max_pairs, max_rounds)
    if height is None:
        if scratch.distance is None:
            scratch.distance = DistanceScratch(1, H, W, labels.device)
        height = distance_transform(labels, sites="edge", max_distance=max_distance, scratch=scratch.distance)["d2"]
        if R:
            height.clamp_(max=R * R)                              # FAR is taken as R * R
    out = torch.empty(H, W, dtype=torch.int32, device=labels.device)
    with torch.cuda.device(labels.device):
        s = _lib.stream_ptr()
        call("insar_split_basins", ptr(labels), ptr(height), H, W, max_pairs, max_rounds, ptr(scratch.scratch), s)

        def first_read(ctrl):
            if ctrl[2]:
                raise InsarError(f"{who}: height is negative on {int(ctrl[2])} foreground pixels")
            if ctrl[1] or ctrl[0] > max_pairs:
                raise InsarError(f"{who}: {'more than ' if ctrl[1] else ''}{int(ctrl[0])} adjacent basin pairs exceed "
                                 f"max_pairs={max_pairs}: raise max_pairs, or smooth the height map")

        rounds, converged, _ = merge_rounds(
            lambda first, n: call("insar_split_rounds", ptr(height), H, W, int(squared), T, first, n, max_pairs, max_rounds,
                                  ptr(scratch.scratch), s),
            scratch.ctrl_host, scratch.ctrl, max_rounds, first_read)
        call("insar_split_finish", ptr(labels), ptr(height), ptr(mask), ptr(conf), H, W, max_regions, max_pairs, max_rounds,
             ptr(scratch.scratch), ptr(scratch.table), ptr(out), s)
        raw = read_back(scratch.host, scratch.table)
    regions = pieces_from_table(raw, W, max_regions, conf is not None)
    return {"labels": out, "regions": regions, "count": int(len(regions["id"])), "raw_basins": int(raw.view(SPLIT_DTYPE)["y0"][0]),
            "rounds": rounds, "converged": converged}
