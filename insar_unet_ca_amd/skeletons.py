"""Centre lines: every region of a device label map thinned to a one-pixel skeleton at once (csrc/skeleton.hip:
insar_skeleton_planes / _step / _stats), the kind of every skeleton pixel, and a table of what one measures on a linear
feature: length, width, orientation, ends and junctions. `ScenePredictor.detect(..., skeletons=True)` thins the regions it
labelled.

Semantics (include/insar_hip.h, "centre lines"): Guo and Hall's two-subiteration thinning per region (a neighbour counts only
if it is alive and carries the pixel's label, so the result is what thinning each region's mask alone would give); kinds
1 isolated, 2 end, 3 line, 4 junction by the number of 0 -> 1 transitions round the pixel. Integers only on the device: every
output is bitwise reproducible. The float table is numpy on those integers.

    out = thin_regions(det["labels"])                  # 2 + ceil(max_iterations / 8) launches, + 2 for the widths; ONE read-back
    out["skeleton"]                                     # uint8 [H, W] on the device, the kinds
    out["table"]["length"], ["mean_width"], ["orientation"]    # float64 per label 1..n
    props = {int(l): {"length": float(v)} for l, v in zip(out["table"]["label"], out["table"]["length"])}
    to_geojson(region_outlines(det["labels"]), properties=props)

Axes: x to the right, y down. `orientation` is the angle of the skeleton's principal axis in degrees in [0, 180), measured from
the +x axis towards +y: a horizontal line is 0, a vertical one 90, a line from the top left to the bottom right 45 and one
from the bottom left to the top right 135.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_map, check_on_device, query_bytes, read_back
from .distance import DistanceScratch, distance_transform
from .regions import DEFAULT_MAX_REGIONS

MAX_DIM = 32767
MAX_ITERATIONS = 32768
ITERATIONS_PER_LAUNCH = 8                # SK_T of csrc/skeleton.hip
ISOLATED, END, LINE, JUNCTION = 1, 2, 3, 4

# the C struct InsarSkeletonStat (include/insar_hip.h); record 0 of a table is the header: n = iterations, n_end = converged,
# n_junction = the largest label, n_orth = the overflow flag
STAT_DTYPE = np.dtype([("sum_y", "<i8"), ("sum_x", "<i8"), ("sum_yy", "<i8"), ("sum_xx", "<i8"), ("sum_xy", "<i8"),
                       ("sum_d2", "<i8"), ("n", "<i4"), ("n_end", "<i4"), ("n_junction", "<i4"), ("n_orth", "<i4"),
                       ("n_diag", "<i4"), ("n_far", "<i4"), ("max_d2", "<i4"), ("_pad", "<i4")])
assert STAT_DTYPE.itemsize == 80
STAT_FIELDS = tuple(f for f in STAT_DTYPE.names if f != "_pad")
TABLE_FIELDS = ("label", "n", "length", "mean_width", "max_width", "orientation", "elongation", "n_end", "n_junction")


def scratch_bytes(H: int, W: int, max_iterations: int = 32, max_regions: int = DEFAULT_MAX_REGIONS):
    """(scratch bytes, table bytes) of an H x W map thinned for max_iterations with max_regions records. Host arithmetic only."""
    return query_bytes("insar_skeleton_scratch_bytes", H, W, max_iterations, max_regions, outputs=2)


def launches(H: int, W: int, max_iterations: int = 32, widths: bool = True) -> int:
    """Kernel launches of one `thin_regions`: 2 + ceil(max_iterations / 8), and the distance transform's 2 with widths."""
    n = call("insar_skeleton_launches", int(H), int(W), int(max_iterations), int(bool(widths)))
    if n < 0:
        raise InsarError(f"insar_skeleton_launches failed ({n}): {_lib.load().insar_last_error().decode(errors='replace')}")
    return n


class SkeletonScratch(Scratch):
    """The device buffers of one (H, W, max_iterations, max_regions): the bit planes and flags, the table, the pinned host copy
    the table is read back into, and the distance transform's scratch once widths have used it. Nothing in them has to survive
    between calls. The skeleton map is the caller's: every call returns a fresh one."""
    KEY, DEVICE_AT = ("H", "W", "max_iterations", "max_regions"), 2

    def __init__(self, H: int, W: int, device, max_iterations: int = 32, max_regions: int = DEFAULT_MAX_REGIONS):
        sb, tb = scratch_bytes(H, W, max_iterations, max_regions)
        super().__init__((H, W, max_iterations, max_regions), device, scratch=sb, table=tb, host=tb)
        self.distance = None

    def distance_scratch(self) -> DistanceScratch:
        if self.distance is None:
            self.distance = DistanceScratch(1, self.H, self.W, self.scratch.device)
        return self.distance


def _check_args(labels, max_iterations, widths, max_regions, scratch):
    """Everything but the device."""
    who = "thin_regions"
    check_map(who, "labels", labels, (torch.int32,))
    H, W = labels.shape
    if H < 1 or W < 1 or H > MAX_DIM or W > MAX_DIM:
        raise InsarError(f"{who}: map {H} x {W}: need 1 <= H, W <= {MAX_DIM}")
    mi = check_int(who, "max_iterations", max_iterations, 1, MAX_ITERATIONS, integral_floats=True)
    if not isinstance(widths, (bool, np.bool_)):
        raise InsarError(f"{who}: widths={widths!r}: True or False")
    max_regions = check_int(who, "max_regions", max_regions, 1, 1 << 30, integral_floats=False)
    if scratch is not None:
        SkeletonScratch.check(who, scratch, (H, W, mi, max_regions), labels.device)
    return int(H), int(W), mi, max_regions


def stats_from_table(raw: np.ndarray, n_labels: int) -> Dict[str, np.ndarray]:
    """The integer arrays (fresh, one entry per label 1..n_labels, plus "label") from the raw bytes of a device table."""
    r = raw.view(STAT_DTYPE)[1:1 + n_labels]
    out = {"label": np.arange(1, n_labels + 1, dtype=np.int32)}
    for f in STAT_FIELDS:
        out[f] = r[f].copy()
    return out


def skeleton_table(raw, *, widths: bool = True) -> Dict[str, np.ndarray]:
    """The table of linear features, float64, from the integer accumulators `raw`: a structured array of STAT_DTYPE or a dict
    of equally long integer arrays with its fields (a "label" entry is passed through, else labels count from 1).

        length       n_orth + sqrt(2) n_diag: the 4-adjacent links plus the diagonal ones no 4-adjacent pair already spans
        mean_width   2 sqrt(sum_d2 / (n - n_far)) + 1, NaN where n == n_far (or without widths); max_width 2 sqrt(max_d2) + 1
        orientation  0.5 atan2(2 mu_xy, mu_xx - mu_yy) in degrees in [0, 180) of the central second moments (x right, y down:
                     0 horizontal, 90 vertical, 45 from the top left to the bottom right); NaN where both eigenvalues are 0
        elongation   sqrt(l1 / l2) of the two eigenvalues l1 >= l2: inf for a straight line, NaN for a single pixel
        n, n_end, n_junction   the integers, unchanged
    Pure numpy; no device."""
    if isinstance(raw, np.ndarray) and raw.dtype.names:
        raw = {f: raw[f] for f in raw.dtype.names}
    g = lambda f: np.asarray(raw[f]).astype(np.float64)
    n = g("n")
    out = {"label": np.asarray(raw["label"]).copy() if "label" in raw else np.arange(1, len(n) + 1, dtype=np.int32),
           "n": np.asarray(raw["n"]).copy()}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["length"] = g("n_orth") + np.sqrt(2.0) * g("n_diag")
        near = n - g("n_far")
        if widths:
            out["mean_width"] = np.where(near > 0, 2.0 * np.sqrt(g("sum_d2") / near) + 1.0, np.nan)
            out["max_width"] = 2.0 * np.sqrt(g("max_d2")) + 1.0
        else:
            out["mean_width"] = np.full(len(n), np.nan)
            out["max_width"] = np.full(len(n), np.nan)
        my, mx = g("sum_y") / n, g("sum_x") / n
        myy = g("sum_yy") / n - my * my
        mxx = g("sum_xx") / n - mx * mx
        mxy = g("sum_xy") / n - mx * my
        half = 0.5 * (mxx + myy)
        root = np.sqrt((0.5 * (mxx - myy)) ** 2 + mxy ** 2)
        l1, l2 = half + root, np.maximum(half - root, 0.0)
        flat = ~(l1 > 0)                                                       # a single pixel, or no pixel at all
        ang = np.degrees(0.5 * np.arctan2(2.0 * mxy, mxx - myy)) % 180.0
        out["orientation"] = np.where(flat, np.nan, np.where(ang >= 180.0, 0.0, ang))
        out["elongation"] = np.where(flat, np.nan, np.sqrt(l1 / l2))
    out["n_end"] = np.asarray(raw["n_end"]).copy()
    out["n_junction"] = np.asarray(raw["n_junction"]).copy()
    return out


def thin_regions(labels: torch.Tensor, *, max_iterations: int = 32, widths: bool = True,
                 max_regions: int = DEFAULT_MAX_REGIONS, scratch: Optional[SkeletonScratch] = None) -> dict:
    """Centre lines of every region of a device label map (int32 [H, W], <= 0 = background).

        out["skeleton"]    device uint8 [H, W]: 0, or the kind 1 isolated, 2 end, 3 line, 4 junction
        out["iterations"]  the iterations that deleted a pixel; out["converged"] = iterations < max_iterations: False says the
                           bound cut the thinning short (or the last allowed iteration happened to finish it), and the
                           skeleton is then the partial image after max_iterations, wider than one pixel in places
        out["stats"]       dict of numpy integer arrays per label 1..n (n = the largest label in the map): "label" and the
                           fields of InsarSkeletonStat
        out["table"]       `skeleton_table(out["stats"])`: length, mean_width, max_width, orientation, elongation, n_end, ...

    With `widths` the exact "edge" distance transform of the label map (max_distance = max_iterations + 2) is sampled on
    the skeleton. A region that touches no other value inside the image (one that fills it) has no edge site: its pixels
    count into n_far and its widths are NaN. 2 + ceil(max_iterations / 8) launches (+ 2 with widths) on the current stream
    whatever the map holds, and ONE read-back, of the table, at the end. A label above `max_regions` raises InsarError.
    `scratch`: a SkeletonScratch of this map size, max_iterations and max_regions to reuse (else allocated)."""
    H, W, mi, max_regions = _check_args(labels, max_iterations, widths, max_regions, scratch)
    check_on_device("thin_regions", "labels", labels)
    if scratch is None:
        scratch = SkeletonScratch(H, W, labels.device, mi, max_regions)
    steps = launches(H, W, mi, False) - 2
    sp, tp = ptr(scratch.scratch), ptr(scratch.table)
    skeleton = torch.empty((H, W), dtype=torch.uint8, device=labels.device)
    with torch.cuda.device(labels.device):
        s = _lib.stream_ptr()
        d2 = None
        if widths:
            d2 = distance_transform(labels, sites="edge", max_distance=mi + 2, scratch=scratch.distance_scratch())["d2"]
        call("insar_skeleton_planes", ptr(labels), H, W, mi, max_regions, sp, tp, s)
        for step in range(steps):
            call("insar_skeleton_step", H, W, mi, step, sp, s)
        call("insar_skeleton_stats", ptr(labels), ptr(d2), H, W, mi, max_regions, sp, tp, ptr(skeleton), s)
        # the header first in the same copy: the records worth reading are bounded by the pixels, whatever max_regions is
        nbytes = STAT_DTYPE.itemsize * (1 + min(max_regions, H * W))
        raw = read_back(scratch.host, scratch.table, nbytes)
    head = raw.view(STAT_DTYPE)[0]
    largest = int(head["n_junction"])
    if int(head["n_orth"]) != 0 or largest > max_regions:
        raise InsarError(f"thin_regions: label {largest} exceeds max_regions={max_regions}: raise max_regions")
    stats = stats_from_table(raw, largest)
    return {"skeleton": skeleton, "iterations": int(head["n"]), "converged": bool(head["n_end"]), "stats": stats,
            "table": skeleton_table(stats, widths=bool(widths))}
