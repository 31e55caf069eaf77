"""Polygon rasterisation: polygons (the list `to_polygons` returns, or a GeoJSON FeatureCollection as `to_geojson` writes it)
become a device label map, uint8 or int32, through csrc/raster.hip (insar_raster_polygons). The inverse of `region_outlines`.

Semantics (include/insar_hip.h, "polygon rasterisation"): vertices are quantised ONCE, on the host, to int32 units of 1/256
pixel on the lattice of `region_outlines` ((0, 0) is the top-left corner of pixel (0, 0)); everything after that is integer
arithmetic. A pixel belongs to a polygon iff its centre is inside by the top-left rule (a centre on a left flank is inside, on
a right flank outside), so polygons that share an edge tile the plane. Where exactly one polygon covers a pixel it gets that
polygon's value; where none does it keeps the background; anything else (overlaps, self-intersections, a hole outside its
exterior) becomes `overlap_value`, the pipeline's void. Integers only: the map is bitwise reproducible.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Union

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_map, inverse_affine, query_bytes

SUBPIXEL = 256                           # fixed-point units per pixel
COORD_LIMIT = 1 << 24                    # |X|, |Y| <= 2^24: every product of the crossing rule fits int64
MAX_WIDTH = 16384
MAX_CROSSINGS = 1 << 30
MAX_EDGES = 1 << 28
_DTYPES = {torch.uint8: _lib.RASTER_U8, torch.int32: _lib.RASTER_I32}


def band_rows(W: int) -> int:
    """Rows of one band (one work-group, two LDS planes) at scene width W: a power of two. Host arithmetic only."""
    r = call("insar_raster_band_rows", int(W))
    if r < 0:
        raise InsarError(f"insar_raster_band_rows failed ({r}): {_lib.load().insar_last_error().decode(errors='replace')}")
    return r


def launches() -> int:
    """Kernel launches of one call, whatever the table holds."""
    return call("insar_raster_launches")


def scratch_bytes(H: int, W: int, max_crossings: int) -> int:
    """Bytes of scratch for an H x W scene with room for max_crossings crossing records. Host arithmetic only."""
    return query_bytes("insar_raster_scratch_bytes", H, W, max_crossings, outputs=1)


def _exact_sum(a: np.ndarray) -> int:
    """Sum of int64 terms as a Python integer, whatever its size."""
    return (int((a >> 20).sum()) << 20) + int((a & ((1 << 20) - 1)).sum())


class PolygonTable:
    """The edge table of a set of polygons: `edges` int32 [n, 5] = (X0, Y0, X1, Y1, value) in 1/256 pixel, no horizontal
    edges, exteriors oriented like the exteriors of `region_outlines` and holes the other way.

        table.edges            numpy, never written after packing
        table.bounds           (Y0, X0, Y1, X1) over the edges in 1/256 pixel, None for an empty table
        table.crossings(H)     the exact number of (edge, row of [0, H)) crossings: the records one call emits
        table.row_value_bound  the largest sum of |value| over the edges crossing any one row
        table.device_edges(d)  the table on device d, uploaded on first use and cached
    """

    def __init__(self, edges: np.ndarray):
        edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 5)
        if len(edges) > MAX_EDGES:
            raise InsarError(f"PolygonTable: {len(edges)} edges, at most 2^28")
        if len(edges) and (edges[:, 1] == edges[:, 3]).any():
            raise InsarError("PolygonTable: horizontal edges (Y0 == Y1) do not belong in the table")
        if len(edges) and int(np.abs(edges[:, :4].astype(np.int64)).max()) > COORD_LIMIT:
            raise InsarError("PolygonTable: a coordinate lies outside +-2^24 (1/256 pixel)")
        self.edges = edges
        self.edges.setflags(write=False)
        y = edges[:, [1, 3]].astype(np.int64)
        self._r0 = (y.min(axis=1) + 127) >> 8                   # ceil((Y - 128) / 256): rows r0 <= r < r1 are crossed
        self._r1 = (y.max(axis=1) + 127) >> 8
        self.bounds = None
        if len(edges):
            x = edges[:, [0, 2]]
            self.bounds = (int(y.min()), int(x.min()), int(y.max()), int(x.max()))
        self._bound = None
        self._device: Dict[torch.device, torch.Tensor] = {}

    def __len__(self) -> int:
        return len(self.edges)

    def crossings(self, H: int) -> int:
        return int((np.clip(self._r1, 0, H) - np.clip(self._r0, 0, H)).sum())

    @property
    def row_value_bound(self) -> int:
        if self._bound is None:
            self._bound = 0
            if len(self.edges):
                v = np.abs(self.edges[:, 4].astype(np.int64))
                rows = np.concatenate([self._r0, self._r1])
                delta = np.concatenate([v, -v])
                order = np.argsort(rows, kind="stable")
                rows, run = rows[order], np.cumsum(delta[order])
                last = np.r_[rows[1:] != rows[:-1], True]       # the running sum once every event of a row is in
                self._bound = int(run[last].max(initial=0))
        return self._bound

    def device_edges(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = torch.from_numpy(np.array(self.edges)).to(device)
        return self._device[device]


def _value_of(values, label) -> int:
    v = label if values is None else values(label) if callable(values) else values.get(label)
    if v is None:
        raise InsarError(f"pack_polygons: values has no entry for label {label!r}")
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -(1 << 31) <= int(v) < (1 << 31):
        raise InsarError(f"pack_polygons: value {v!r} of label {label!r} is not an int32")
    return int(v)


def _quantise(ring, inverse) -> np.ndarray:
    """A ring as int64 [n, 2] = (Y, X) in 1/256 pixel: (y, x) as given without a transform, else the inverse affine of world
    (x, y), in float64; then np.rint(v * 256)."""
    r = np.asarray(ring, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != 2:
        raise InsarError(f"pack_polygons: a ring must be an [n, 2] array, got shape {r.shape}")
    if inverse is not None:
        inv, t = inverse
        r = ((r - t) @ inv.T)[:, ::-1]                          # world (x, y) -> pixel (x, y) -> (y, x)
    q = np.rint(r * SUBPIXEL)
    if not np.isfinite(q).all() or (np.abs(q) > COORD_LIMIT).any():
        raise InsarError("pack_polygons: a vertex lies outside +-2^24 / 256 = +-65536 pixels of the scene origin")
    return q.astype(np.int64)


def _ring_edges(q: np.ndarray, hole: bool, value: int) -> Optional[np.ndarray]:
    """Edges of one quantised ring (closed or open), oriented by the sign of its doubled area; None for a zero-area ring."""
    if len(q) < 3:
        return None
    n = np.roll(q, -1, axis=0)
    area2 = _exact_sum(q[:, 1] * n[:, 0] - n[:, 1] * q[:, 0])   # x_i y_{i+1} - x_{i+1} y_i, as the outlines' area2
    if area2 == 0:
        return None
    if (area2 < 0) != hole:                                     # exteriors positive, holes negative
        q = q[::-1]
        n = np.roll(q, -1, axis=0)
    keep = q[:, 0] != n[:, 0]
    e = np.empty((int(keep.sum()), 5), dtype=np.int32)
    e[:, 0], e[:, 1], e[:, 2], e[:, 3], e[:, 4] = q[keep, 1], q[keep, 0], n[keep, 1], n[keep, 0], value
    return e


def pack_polygons(polygons: List[dict], *, transform=None, values: Union[None, dict, Callable] = None) -> PolygonTable:
    """The edge table of `polygons`, the list form `to_polygons` returns: [{"label", "polygons": [{"exterior": [n, 2],
    "holes": [[n, 2], ...]}, ...]}, ...]. Rings are closed or open, in any orientation and from any start vertex; vertices are
    (y, x) in pixels without `transform`, world (x, y) with the 2 x 3 affine that `to_polygons(transform=)` applied, which is
    inverted here in float64. `values`: label -> burnt value as a dict or a callable, None for the label itself.
    Vertices outside the scene are legal; one further than 65536 pixels from the origin raises InsarError. Zero-area rings
    and horizontal edges are dropped."""
    inverse = None if transform is None else inverse_affine(transform)
    parts = []
    for entry in polygons:
        value = _value_of(values, entry["label"])
        for poly in entry["polygons"]:
            for hole, ring in [(False, poly["exterior"])] + [(True, h) for h in poly.get("holes", ())]:
                e = _ring_edges(_quantise(ring, inverse), hole, value)
                if e is not None and len(e):
                    parts.append(e)
    return PolygonTable(np.concatenate(parts, axis=0) if parts else np.zeros((0, 5), dtype=np.int32))


def from_geojson(fc: dict, *, transform=None, value_property: str = "label", values=None) -> PolygonTable:
    """The edge table of a GeoJSON FeatureCollection (or a single Feature) of Polygon / MultiPolygon geometries, the inverse
    of `to_geojson`: coordinates are [x, y], lattice x, y without `transform`, world coordinates with it. The label of a
    feature is properties[value_property]; `values` as in `pack_polygons`."""
    feats = fc["features"] if fc.get("type") == "FeatureCollection" else [fc]
    entries = []
    for f in feats:
        geom = f.get("geometry") or {}
        kind = geom.get("type")
        if kind == "Polygon":
            polys = [geom["coordinates"]]
        elif kind == "MultiPolygon":
            polys = geom["coordinates"]
        else:
            raise InsarError(f"from_geojson: geometry type {kind!r}: Polygon or MultiPolygon")
        props = f.get("properties") or {}
        if value_property not in props:
            raise InsarError(f"from_geojson: a feature has no property {value_property!r}")
        out = []
        for rings in polys:
            arr = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings]
            if transform is None:
                arr = [a[:, ::-1] for a in arr]                 # [x, y] -> (y, x)
            if arr:
                out.append({"exterior": arr[0], "holes": arr[1:]})
        entries.append({"label": props[value_property], "polygons": out})
    return pack_polygons(entries, transform=transform, values=values)


class RasterScratch(Scratch):
    """The device scratch of one (H, W) with room for `max_crossings` crossing records. Nothing in it has to survive between
    calls. The label map and the overlap count are the caller's: every call returns fresh ones."""
    KEY, DEVICE_AT = ("H", "W", "max_crossings"), 2

    def __init__(self, H: int, W: int, device, max_crossings: int):
        super().__init__((H, W, max_crossings), device, scratch=scratch_bytes(H, W, max_crossings))


def rasterise_polygons(table: PolygonTable, H: int, W: int, *, dtype: torch.dtype = torch.uint8, fill: int = 0,
                       overlap_value: int = 255, base: Optional[torch.Tensor] = None, device=None,
                       scratch: Optional[RasterScratch] = None) -> dict:
    """Burn a PolygonTable into a device label map.

        out = rasterise_polygons(table, H, W)                   # uint8: a class map for SceneCrops / evaluate
        out["labels"]          device `dtype` [H, W]
        out["overlap_pixels"]  device int64 scalar: the pixels that became overlap_value because the polygons disagree

    A pixel no polygon covers is `fill`, or the pixel of `base` (a contiguous device tensor [H, W] of `dtype`, not written)
    when given; one covered exactly once takes the polygon's value if `dtype` holds it and it is not overlap_value;
    everything else is overlap_value. dtype: torch.uint8 or torch.int32. Five launches on the current stream, no read-back.
    `scratch`: a RasterScratch of this scene size with room for table.crossings(H) records (else allocated)."""
    if not isinstance(table, PolygonTable):
        raise InsarError(f"rasterise_polygons: table must be a PolygonTable, got {type(table).__name__}")
    if dtype not in _DTYPES:
        raise InsarError(f"rasterise_polygons: dtype {dtype}: torch.uint8 or torch.int32")
    who = "rasterise_polygons"
    H, W = (check_int(who, n, v, 1, (1 << 31) - 1, integral_floats=False) for n, v in (("H", H), ("W", W)))
    if W > MAX_WIDTH:
        raise InsarError(f"rasterise_polygons: scene width {W} above {MAX_WIDTH}")
    if H * W >= 1 << 31:
        raise InsarError(f"rasterise_polygons: scene {H} x {W} has 2^31 pixels or more")
    lo, hi = (0, 255) if dtype == torch.uint8 else (-(1 << 31), (1 << 31) - 1)
    fill, overlap_value = (check_int(who, n, v, lo, hi, integral_floats=False) for n, v in (("fill", fill), ("overlap_value", overlap_value)))
    if table.row_value_bound >= 1 << 31:
        raise InsarError(f"rasterise_polygons: the values of the edges crossing one row sum to {table.row_value_bound} in "
                         f"magnitude: 2^31 or more leaves the int32 sums of the kernels")
    n_cross = table.crossings(H)
    if n_cross > MAX_CROSSINGS:
        raise InsarError(f"rasterise_polygons: {n_cross} edge-row crossings, at most 2^30")
    if base is not None:
        check_map(who, "base", base, (dtype,), shape=(H, W), of="the scene")
        if device is not None and torch.device(device) != base.device:
            raise InsarError(f"rasterise_polygons: base lives on {base.device}, device={device}")
        device = base.device
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise InsarError("rasterise_polygons: needs a ROCm device (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if scratch is None:
        scratch = RasterScratch(H, W, device, n_cross)
    elif (scratch.H, scratch.W) != (H, W) or scratch.scratch.device != device or scratch.max_crossings < n_cross:
        raise InsarError(f"rasterise_polygons: scratch of {scratch.H} x {scratch.W} with {scratch.max_crossings} records on "
                         f"{scratch.scratch.device} for a {H} x {W} scene with {n_cross} crossings on {device}")
    labels = torch.empty(H, W, dtype=dtype, device=device)
    overlap = torch.empty((), dtype=torch.int64, device=device)
    edges = table.device_edges(device) if len(table) else None
    with torch.cuda.device(device):
        call("insar_raster_polygons", ptr(edges), len(table), H, W, scratch.max_crossings, _DTYPES[dtype], fill, overlap_value,
             ptr(base), ptr(labels), ptr(scratch.scratch), ptr(overlap), _lib.stream_ptr())
    return {"labels": labels, "overlap_pixels": overlap}


def labels_from_geojson(fc: dict, H: int, W: int, *, transform=None, value_property: str = "label", values=None, **kw) -> torch.Tensor:
    """GeoJSON annotations to a device label map in one call: from_geojson + rasterise_polygons(**kw). The uint8 default goes
    unchanged into SceneCrops(labels=...) and ScenePredictor.evaluate(scene, gt_mask)."""
    table = from_geojson(fc, transform=transform, value_property=value_property, values=values)
    return rasterise_polygons(table, H, W, **kw)["labels"]
