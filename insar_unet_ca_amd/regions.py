"""Regions of a class map: connected-component labelling, per-region statistics and a minimum-area / minimum-confidence
filter on the device (csrc/regions.hip: insar_regions_tiles / _merge / _flatten / _number / _relabel), the last stage of
the whole-scene inference path: `ScenePredictor.detect` is `predict` followed by `label_regions`.

Semantics: a pixel is foreground if mask != 0 and (with `conf`) conf >= min_conf; foreground pixels are connected if they are
4- / 8-neighbours and carry the same class; a region's root is its smallest row-major pixel index; regions of at least
`min_area` pixels are kept and numbered 1..N in ascending root order (`scipy.ndimage.label`'s numbering). Everything is
bitwise reproducible: the per-region accumulators are integers (int64 area / sum y / sum x, min / max box, confidence as the
sum of llrint(clamp(conf, 0, 1) * 2^30)); the float fields of the table are formed on the host in float64.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_map, check_on_device, query_bytes, read_back

CONF_SCALE = 1 << 30
DEFAULT_MAX_REGIONS = 65536

# the C struct InsarRegion (include/insar_hip.h); record 0 of a table is the header, whose `area` is the count N
REGION_DTYPE = np.dtype([("area", "<i8"), ("sum_y", "<i8"), ("sum_x", "<i8"), ("sum_conf", "<i8"),
                         ("y0", "<i4"), ("x0", "<i4"), ("y1", "<i4"), ("x1", "<i4"),
                         ("root", "<i4"), ("cls", "<i4"), ("_pad", "<i4", (2,))])
assert REGION_DTYPE.itemsize == 64


def scratch_bytes(H: int, W: int, max_regions: int = DEFAULT_MAX_REGIONS):
    """(scratch bytes, table bytes) of an H x W scene with room for max_regions regions. Host arithmetic only."""
    return query_bytes("insar_regions_scratch_bytes", H, W, max_regions, outputs=2)


class RegionScratch(Scratch):
    """The device buffers of one (H, W, max_regions): scene-sized scratch, the region table, and the pinned host copy the
    table is read back into. Nothing in them has to survive between calls."""
    KEY, SHOW, DEVICE_AT = ("H", "W", "max_regions"), "{} x {}, max_regions={}", 2

    def __init__(self, H: int, W: int, device: torch.device, max_regions: int = DEFAULT_MAX_REGIONS):
        sb, tb = scratch_bytes(H, W, max_regions)
        super().__init__((H, W, max_regions), device, scratch=sb, table=tb, host=tb)


def _check_args(mask, conf, connectivity, min_area, min_conf, max_regions) -> None:
    who = "label_regions"
    check_on_device(who, "mask", mask)
    check_map(who, "mask", mask, (torch.uint8,))
    H, W = mask.shape
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise InsarError(f"{who}: scene {H} x {W}: need H, W >= 1 and H * W < 2^31")
    if conf is not None:
        check_on_device(who, "conf", conf, like=mask)
        check_map(who, "conf", conf, (torch.float32,), shape=(H, W), of="mask")
    if connectivity not in (4, 8):
        raise InsarError(f"connectivity={connectivity!r}: 4 or 8")
    check_int(who, "min_area", min_area, 1, integral_floats=True)
    check_int(who, "max_regions", max_regions, 1, integral_floats=True)
    if not np.isfinite(np.float32(min_conf)):
        raise InsarError(f"min_conf={min_conf!r}: a finite number")


def _launch(mask: torch.Tensor, conf: Optional[torch.Tensor], connectivity: int, min_area: int, min_conf: float,
            max_regions: int, scratch: torch.Tensor, table: torch.Tensor, labels: torch.Tensor, mask_out: torch.Tensor) -> None:
    """The five phase calls (seven launches) on the current stream. `table` holds 64 * (1 + max_regions) bytes."""
    H, W = mask.shape
    s = _lib.stream_ptr()
    call("insar_regions_tiles", ptr(mask), ptr(conf), float(min_conf), H, W, connectivity, ptr(scratch), s)
    call("insar_regions_merge", ptr(mask), H, W, connectivity, ptr(scratch), s)
    call("insar_regions_flatten", H, W, ptr(scratch), s)
    call("insar_regions_number", ptr(mask), H, W, int(min_area), max_regions, ptr(scratch), ptr(table), s)
    call("insar_regions_relabel", ptr(mask), ptr(conf), H, W, max_regions, ptr(scratch), ptr(table), ptr(labels), ptr(mask_out), s)


def regions_from_table(raw: np.ndarray, max_regions: int, with_conf: bool) -> Dict[str, np.ndarray]:
    """The host table (fresh arrays) from the raw bytes of a device table: raises if the count in the header exceeds
    max_regions."""
    rec = raw.view(REGION_DTYPE)
    n = int(rec["area"][0])
    if n > max_regions:
        raise InsarError(f"label_regions: {n} regions exceed max_regions={max_regions}: raise max_regions, min_area or min_conf")
    r = rec[1:1 + n]
    area = r["area"].astype(np.int64)
    out = {"id": np.arange(1, n + 1, dtype=np.int32), "cls": r["cls"].astype(np.int32), "area": area,
           "y0": r["y0"].copy(), "x0": r["x0"].copy(), "y1": r["y1"].copy(), "x1": r["x1"].copy(),
           "cy": r["sum_y"].astype(np.float64) / area, "cx": r["sum_x"].astype(np.float64) / area}
    if with_conf:
        out["mean_conf"] = r["sum_conf"].astype(np.float64) / (area.astype(np.float64) * CONF_SCALE)
    return out


def label_regions(mask: torch.Tensor, conf: Optional[torch.Tensor] = None, *, connectivity: int = 8, min_area: int = 1,
                  min_conf: float = 0.0, max_regions: int = DEFAULT_MAX_REGIONS, scratch: Optional[RegionScratch] = None) -> dict:
    """Connected regions of a device class map.

        out = label_regions(mask, conf, connectivity=8, min_area=20, min_conf=0.6)
        out["labels"]  int32 [H, W]  0 or the region id 1..N     out["mask"]  uint8 [H, W]  the class map, dropped pixels 0
        out["count"]   N                                         out["regions"]  dict of numpy arrays of length N:
        id, cls, area (int64), y0, x0, y1, x1 (half-open box), cy, cx (float64)[, mean_conf (float64) with conf]

    Seven launches on the current stream and ONE device-to-host read-back (the count together with the table). More than
    `max_regions` kept regions raise InsarError. `scratch`: a RegionScratch of this scene size to reuse (else allocated)."""
    _check_args(mask, conf, connectivity, min_area, min_conf, max_regions)
    H, W = mask.shape
    max_regions = int(max_regions)
    if scratch is None:
        scratch = RegionScratch(H, W, mask.device, max_regions)
    else:
        RegionScratch.check("label_regions", scratch, (H, W, max_regions), mask.device)
    labels = torch.empty(H, W, dtype=torch.int32, device=mask.device)
    mask_out = torch.empty(H, W, dtype=torch.uint8, device=mask.device)
    with torch.cuda.device(mask.device):
        _launch(mask, conf, int(connectivity), int(min_area), float(np.float32(min_conf)), max_regions, scratch.scratch,
                scratch.table, labels, mask_out)
        raw = read_back(scratch.host, scratch.table)
    regions = regions_from_table(raw, max_regions, conf is not None)
    return {"labels": labels, "mask": mask_out, "count": int(len(regions["id"])), "regions": regions}
