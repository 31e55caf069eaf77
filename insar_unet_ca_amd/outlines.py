"""Region outlines: the exact pixel-edge ("crack") outline of every region of a device label map as ordered, closed rings of
lattice vertices, with holes (csrc/outline.hip: insar_outline_edges / _lead / _rank / _rings / _write), and the host helpers that
turn the rings into polygons and GeoJSON. `ScenePredictor.detect(..., outlines=True)` traces the regions it labelled.

Semantics (include/insar_hip.h, "region outlines"): vertex (y, x) is the top-left corner of pixel (y, x); a boundary edge is a
side of a labelled pixel whose neighbour across it differs, directed with the region on its right; a ring is one cycle of the
successor map, led by its smallest edge id 4 * pixel + side, rings in ascending leader order; exteriors have positive doubled
area `area2`, holes negative. At a saddle the ring turns left with connectivity 8 and right with connectivity 4, so a map
labelled by `label_regions` with the same connectivity gives every region exactly one exterior ring. Integers only: every
output is bitwise reproducible.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_map, check_on_device, query_bytes, read_back

DEFAULT_MAX_RINGS = 65536
DEFAULT_MAX_VERTICES = 1 << 22
DEFAULT_MAX_EDGES = 1 << 22
MAX_PIXELS = 1 << 29                     # edge ids are 4 * pixel + side in an int32

# the C struct InsarRing (include/insar_hip.h); record 0 of a table is the header: label = R, count = V, edges = E
RING_DTYPE = np.dtype([("area2", "<i8"), ("label", "<i4"), ("leader", "<i4"), ("start", "<i4"), ("count", "<i4"),
                       ("edges", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("y1", "<i4"), ("x1", "<i4"), ("_pad", "<i4")])
assert RING_DTYPE.itemsize == 48
RING_FIELDS = ("ring", "label", "start", "count", "edges", "area2", "hole", "y0", "x0", "y1", "x1")


def scratch_bytes(H: int, W: int, max_rings: int = DEFAULT_MAX_RINGS, max_edges: int = DEFAULT_MAX_EDGES):
    """(scratch bytes, table bytes) of an H x W scene with max_edges edge slots and max_rings rings. Host arithmetic only."""
    return query_bytes("insar_outline_scratch_bytes", H, W, max_rings, max_edges, outputs=2)


def launches(n_edges: int) -> int:
    """Kernel launches of one call for n_edges boundary edges: 12 + 2 ceil(log2 n_edges)."""
    return call("insar_outline_launches", int(n_edges))


class OutlineScratch(Scratch):
    """The device buffers of one (H, W, max_rings, max_vertices, max_edges): scratch, the ring table, and the pinned host
    copy the table is read back into. Nothing in them has to survive between calls. The vertex array is the caller's: every
    call returns a fresh one."""
    KEY, DEVICE_AT = ("H", "W", "max_rings", "max_vertices", "max_edges"), 2

    def __init__(self, H: int, W: int, device: torch.device, max_rings: int = DEFAULT_MAX_RINGS,
                 max_vertices: int = DEFAULT_MAX_VERTICES, max_edges: int = DEFAULT_MAX_EDGES):
        sb, tb = scratch_bytes(H, W, max_rings, max_edges)
        super().__init__((H, W, max_rings, max_vertices, max_edges), device, scratch=sb, table=tb, host=tb)


def _check_args(labels, connectivity, max_rings, max_vertices, max_edges) -> None:
    who = "region_outlines"
    check_map(who, "labels", labels, (torch.int32,))
    H, W = labels.shape
    if H < 1 or W < 1 or H * W >= MAX_PIXELS:
        raise InsarError(f"{who}: scene {H} x {W}: need H, W >= 1 and H * W < 2^29")
    if connectivity not in (4, 8):
        raise InsarError(f"connectivity={connectivity!r}: 4 or 8")
    for name, v in (("max_rings", max_rings), ("max_vertices", max_vertices), ("max_edges", max_edges)):
        check_int(who, name, v, 1, 1 << 30, integral_floats=False)
    check_on_device(who, "labels", labels)


def rings_from_table(raw: np.ndarray, n_rings: int) -> Dict[str, np.ndarray]:
    """The host ring table (fresh arrays) from the raw bytes of a device table holding n_rings rings."""
    r = raw.view(RING_DTYPE)[1:1 + n_rings]
    out = {"ring": np.arange(n_rings, dtype=np.int32)}
    for f in ("label", "start", "count", "edges", "area2", "y0", "x0", "y1", "x1", "leader"):
        out[f] = r[f].copy()
    out["hole"] = out["area2"] < 0
    return out


def _empty(device, edge_count: int = 0) -> dict:
    rings = {f: np.zeros(0, dtype=np.int64 if f == "area2" else np.bool_ if f == "hole" else np.int32)
             for f in RING_FIELDS + ("leader",)}
    return {"vertices": torch.empty(0, 2, dtype=torch.int32, device=device), "rings": rings, "ring_count": 0,
            "vertex_count": 0, "edge_count": edge_count}


def region_outlines(labels: torch.Tensor, *, connectivity: int = 8, corners_only: bool = True,
                    max_rings: int = DEFAULT_MAX_RINGS, max_vertices: int = DEFAULT_MAX_VERTICES,
                    max_edges: int = DEFAULT_MAX_EDGES, scratch: Optional[OutlineScratch] = None) -> dict:
    """Outlines of every region of a device label map (int32 [H, W], 0 = background).

        out = region_outlines(det["labels"], connectivity=8)
        out["vertices"]  device int32 [V, 2] as (y, x), ring after ring
        out["rings"]     dict of numpy arrays of length R: ring, label, start, count (the ring's slice of the vertex array),
                         edges (crack length), area2 (int64, negative for holes), hole, y0, x0, y1, x1 (half-open vertex box),
                         leader (smallest edge id)
        out["ring_count"], out["vertex_count"], out["edge_count"]

    `corners_only` keeps the vertices where the outline turns; without it every lattice vertex on the outline is written
    (count == edges). 12 + 2 ceil(log2 E) launches on the current stream and TWO device-to-host read-backs: the edge count E,
    which sizes the doubling rounds, then the ring table. More edges, rings or vertices than the capacities raise InsarError.
    `scratch`: an OutlineScratch of this scene size and these capacities to reuse (else allocated)."""
    _check_args(labels, connectivity, max_rings, max_vertices, max_edges)
    H, W = labels.shape
    max_rings, max_vertices, max_edges = int(max_rings), int(max_vertices), int(max_edges)
    if scratch is None:
        scratch = OutlineScratch(H, W, labels.device, max_rings, max_vertices, max_edges)
    else:
        OutlineScratch.check("region_outlines", scratch, (H, W, max_rings, max_vertices, max_edges), labels.device)
    sp, tp = ptr(scratch.scratch), ptr(scratch.table)
    with torch.cuda.device(labels.device):
        s = _lib.stream_ptr()
        call("insar_outline_edges", ptr(labels), H, W, int(connectivity), max_edges, sp, tp, s)
        E = int(read_back(scratch.host, scratch.table, RING_DTYPE.itemsize).view(RING_DTYPE)["edges"][0])
        if E > max_edges:
            raise InsarError(f"region_outlines: {E} boundary edges exceed max_edges={max_edges}: raise max_edges or min_area")
        if E == 0:
            return _empty(labels.device)
        # vertices: E is an upper bound of V, so the array is never larger than the outline itself
        vcap = min(max_vertices, E)
        vertices = torch.empty(vcap, 2, dtype=torch.int32, device=labels.device)
        call("insar_outline_lead", H, W, E, max_edges, sp, s)
        call("insar_outline_rank", H, W, E, max_edges, sp, s)
        call("insar_outline_rings", ptr(labels), H, W, E, max_rings, max_edges, sp, tp, s)
        call("insar_outline_write", H, W, E, int(bool(corners_only)), max_rings, vcap, max_edges, sp, tp, ptr(vertices), s)
        # a ring has four edges or more: R <= E / 4 bounds the records worth copying, whatever max_rings is
        nbytes = RING_DTYPE.itemsize * (1 + min(max_rings, E // 4))
        raw = read_back(scratch.host, scratch.table, nbytes)
    head = raw.view(RING_DTYPE)[0]
    R, V = int(head["label"]), int(head["count"])
    if R > max_rings:
        raise InsarError(f"region_outlines: {R} rings exceed max_rings={max_rings}: raise max_rings or min_area")
    if V > max_vertices:
        raise InsarError(f"region_outlines: {V} vertices exceed max_vertices={max_vertices}: raise max_vertices or min_area")
    return {"vertices": vertices[:V], "rings": rings_from_table(raw, R), "ring_count": R, "vertex_count": V, "edge_count": E}


def perimeters(rings: Dict[str, np.ndarray], ids: np.ndarray) -> np.ndarray:
    """int64 per id of `ids` (region ids >= 0): the sum of `edges` over the rings carrying that label, 0 where there is none."""
    ids = np.asarray(ids, dtype=np.int64)
    total = np.zeros(max(int(ids.max(initial=0)), int(rings["label"].max(initial=0))) + 1, dtype=np.int64)
    np.add.at(total, rings["label"], rings["edges"])
    return total[ids]


# ---- host side: polygons -------------------------------------------------------------------------------------------------------
def _inside(ring: np.ndarray, py: float, px: float) -> bool:
    """Even-odd: crossings of the ray from (py, px) towards -x with the ring's vertical segments (ring [n, 2] as (y, x))."""
    nxt = np.roll(ring, -1, axis=0)
    vert = ring[:, 1] == nxt[:, 1]
    lo, hi = np.minimum(ring[:, 0], nxt[:, 0]), np.maximum(ring[:, 0], nxt[:, 0])
    return bool((vert & (ring[:, 1] < px) & (lo < py) & (py < hi)).sum() & 1)


def _apply(ring_yx: np.ndarray, transform) -> np.ndarray:
    """Close the ring; (y, x) lattice vertices unchanged without a transform, else world = A @ (x, y, 1)."""
    r = np.concatenate([ring_yx, ring_yx[:1]], axis=0)
    if transform is None:
        return r
    A = np.asarray(transform, dtype=np.float64)
    if A.shape != (2, 3):
        raise InsarError(f"transform must be a 2 x 3 affine, got shape {A.shape}")
    xy1 = np.stack([r[:, 1], r[:, 0], np.ones(len(r))], axis=1).astype(np.float64)
    return xy1 @ A.T


def to_polygons(outlines: dict, *, transform=None, drop_collapsed: bool = True) -> List[dict]:
    """One entry per label, in ascending label order: {"label", "polygons": [{"exterior": ndarray [n, 2], "holes": [ndarray,
    ...]}, ...]}, polygons in ring order. Every hole goes to the exterior ring of its label that contains it: the only one
    where there is one, else the smallest (by |area2|) exterior that holds, by an even-odd crossing test, the centre of the
    pixel below-right of the hole's top-left-most vertex, which lies inside the hole. Rings are closed by repeating the first
    vertex. Without `transform` the vertices are the integer lattice (y, x); with a 2 x 3 affine they are float64 world
    coordinates A @ (x, y, 1). A dict with a `collapsed` ring field (`simplify_outlines` writes one) tells exteriors from holes
    by its `hole` field, since a simplified ring may have lost its area, and with `drop_collapsed` leaves collapsed rings out: a
    collapsed exterior takes its holes with it, and a label left without a polygon has no entry. A dict without that field is
    treated exactly as before, whatever `drop_collapsed` says."""
    rings = outlines["rings"]
    v = outlines["vertices"]
    v = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    by_label: Dict[int, dict] = {}
    n = len(rings["label"])
    raw = [v[int(rings["start"][i]):int(rings["start"][i]) + int(rings["count"][i])] for i in range(n)]
    simplified = "collapsed" in rings
    is_ext = ~np.asarray(rings["hole"], dtype=bool) if simplified else np.asarray(rings["area2"]) > 0
    is_hole = np.asarray(rings["hole"], dtype=bool) if simplified else np.asarray(rings["area2"]) < 0
    gone = np.asarray(rings["collapsed"], dtype=bool) if simplified and drop_collapsed else np.zeros(n, dtype=bool)
    for i in range(n):
        if is_ext[i]:
            e = by_label.setdefault(int(rings["label"][i]), {"label": int(rings["label"][i]), "polygons": [], "_ext": []})
            e["polygons"].append({"exterior": _apply(raw[i], transform), "holes": []})
            e["_ext"].append(i)
    for i in range(n):
        if not is_hole[i] or gone[i]:
            continue
        lab = int(rings["label"][i])
        if lab not in by_label:
            raise InsarError(f"to_polygons: ring {i} is a hole of label {lab}, which has no exterior ring")
        ext = by_label[lab]["_ext"]
        pick = 0
        if len(ext) > 1:
            top = raw[i][np.lexsort((raw[i][:, 1], raw[i][:, 0]))[0]]
            py, px = top[0] + 0.5, top[1] + 0.5
            holding = [j for j, r in enumerate(ext) if not gone[r] and _inside(raw[r], py, px)]
            if not holding:
                if any(gone[r] for r in ext):                                 # its exterior collapsed: the hole goes with it
                    continue
                raise InsarError(f"to_polygons: no exterior ring of label {lab} contains hole ring {i}")
            pick = min(holding, key=lambda j: abs(int(rings["area2"][ext[j]])))
        by_label[lab]["polygons"][pick]["holes"].append(_apply(raw[i], transform))
    out = []
    for lab in sorted(by_label):
        e = by_label[lab]
        e["polygons"] = [p for p, r in zip(e["polygons"], e["_ext"]) if not gone[r]]
        del e["_ext"]
        if e["polygons"]:
            out.append(e)
    return out


def to_geojson(outlines: dict, *, transform=None, properties=None, drop_collapsed: bool = True) -> dict:
    """A GeoJSON FeatureCollection: one Polygon / MultiPolygon feature per label, coordinates as [x, y] lists (lattice x, y
    without `transform`, world coordinates with it), rings closed. `properties`: a dict label -> dict merged into the
    feature's properties next to "label", or a callable label -> dict. json-serialisable types only. `drop_collapsed` goes to
    `to_polygons`."""
    feats = []
    for e in to_polygons(outlines, transform=transform, drop_collapsed=drop_collapsed):
        polys = []
        for p in e["polygons"]:
            rings = [p["exterior"]] + p["holes"]
            if transform is None:
                rings = [r[:, ::-1] for r in rings]                     # (y, x) -> [x, y]
            polys.append([[[c.item() for c in pt] for pt in r] for r in rings])
        props = {"label": int(e["label"])}
        extra = properties(e["label"]) if callable(properties) else (properties or {}).get(e["label"])
        if extra:
            props.update(extra)
        geom = {"type": "Polygon", "coordinates": polys[0]} if len(polys) == 1 else {"type": "MultiPolygon", "coordinates": polys}
        feats.append({"type": "Feature", "properties": props, "geometry": geom})
    return {"type": "FeatureCollection", "features": feats}
