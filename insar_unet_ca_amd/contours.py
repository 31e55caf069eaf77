"""Contour lines: the iso-lines of a device raster at up to 32 levels as ordered polylines of sub-pixel vertices, closed rings
and open lines (csrc/contour.hip: insar_contour_edges / _lead / _rank / _lines / _write), and the host helpers that turn them
into coordinates, polygons and GeoJSON. `ScenePredictor.detect(..., contours=dict(levels=...))` contours a probability plane
or a co-registered raster. `simplify_contours` thins the lines on the device (csrc/contour_simplify.hip:
insar_contour_simplify_setup / _rounds / _finish): Douglas-Peucker in exact integers, open lines and rings alike, and the
result has the shape of the `contour_lines` dict, so the host helpers take it unchanged.

Semantics (include/insar_hip.h, "contour lines"): marching squares in exact integers. Every pixel becomes an integer q by
`zonal`'s rule; a node is a pixel centre, at (y + 1/2, x + 1/2) in the frame of `region_outlines`, and every coordinate is an
int32 in 1/256 pixel. A node is above level l iff q >= q_l. A lattice edge between two valid nodes of which exactly one is
above is crossed at s = floor(((q_l - q_below) * 512 + d) / (2 d)) / 256 from its below end, clamped to 1..255, so no vertex
lies on a node. A cell of four valid nodes emits the segments of its above-mask with the above side on the right; a saddle
joins its above corners iff the four q sum to >= 4 q_l. The components are closed rings, led by their smallest crossing id
(l * H * W + p) * 2 + o, and open lines, led by their head; lines come in ascending leader order. Integers only behind the
quantisation: every output is bitwise reproducible.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import MAX_TOLERANCE, ROUNDS_PER_READ  # noqa: F401  (the tools read them from here)
from ._scene import (DEFAULT_MAX_ROUNDS, MAX_ROUNDS, Scratch, check_int, check_map, check_on_device, check_tolerance, pinned,
                     query_bytes, read_back, simplify_rounds)
from .zonal import quantise_scalar

DEFAULT_MAX_LINES = 65536
DEFAULT_MAX_VERTICES = 1 << 22
MAX_LEVELS = 32
MAX_SIDE = 1 << 22                       # 256 * side + 128 fits an int32
MAX_CELLS = 1 << 30                      # crossing ids are (level * H * W + pixel) * 2 + o in an int32
SUBPIXEL = 256

# the C struct InsarContourLine (include/insar_hip.h); records 0..3 of a table are the header, 48 int32 slots
LINE_DTYPE = np.dtype([("area2", "<i8"), ("level", "<i4"), ("leader", "<i4"), ("start", "<i4"), ("count", "<i4"),
                       ("closed", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("y1", "<i4"), ("x1", "<i4"), ("_pad", "<i4")])
assert LINE_DTYPE.itemsize == 48
HEADER_RECORDS = 4
HDR_LINES, HDR_CROSSINGS, HDR_VERTICES, HDR_LEVELS = 2, 3, 5, 16
LINE_FIELDS = ("line", "level", "closed", "start", "count", "leader", "area2", "y0", "x0", "y1", "x1")

_ELEM = {torch.float32: _lib.ZONAL_F32, torch.uint8: _lib.ZONAL_U8, torch.int32: _lib.ZONAL_I32}


def scratch_bytes(H: int, W: int, n_levels: int = 1, max_lines: int = DEFAULT_MAX_LINES, max_vertices: int = DEFAULT_MAX_VERTICES):
    """(scratch bytes, table bytes) of an H x W raster at n_levels levels with max_vertices crossing slots and max_lines lines.
    Host arithmetic only."""
    return query_bytes("insar_contour_scratch_bytes", H, W, n_levels, max_lines, max_vertices, outputs=2)


def launches(n_crossings: int) -> int:
    """Kernel launches of one call that finds n_crossings crossings: 11 + 2 ceil(log2 n_crossings), 5 when there is none."""
    return call("insar_contour_launches", int(n_crossings))


class ContourScratch(Scratch):
    """The device buffers of one (H, W, n_levels, max_lines, max_vertices): scratch, the line table, and the pinned host copy
    the table is read back into. Nothing in them has to survive between calls. The vertex array is the caller's: every call
    returns a fresh one."""
    KEY, DEVICE_AT = ("H", "W", "n_levels", "max_lines", "max_vertices"), 2

    def __init__(self, H: int, W: int, device: torch.device, n_levels: int = 1, max_lines: int = DEFAULT_MAX_LINES,
                 max_vertices: int = DEFAULT_MAX_VERTICES):
        sb, tb = scratch_bytes(H, W, n_levels, max_lines, max_vertices)
        super().__init__((H, W, n_levels, max_lines, max_vertices), device, scratch=sb, table=tb, host=tb)


def quantise_levels(levels, scale: float, is_float: bool) -> np.ndarray:
    """int32 [L]: the levels as the device compares them, by `zonal.quantise_scalar` (scale 1 for an integer raster); refused
    unless they are 1..32 finite numbers that are strictly increasing after quantisation."""
    who = "contour_lines"
    try:
        lv = [float(v) for v in (levels if isinstance(levels, (list, tuple, np.ndarray)) else [levels])]
    except (TypeError, ValueError):
        raise InsarError(f"{who}: levels={levels!r}: 1..{MAX_LEVELS} finite numbers") from None
    if not 1 <= len(lv) <= MAX_LEVELS or not all(math.isfinite(v) for v in lv):
        raise InsarError(f"{who}: levels={levels!r}: 1..{MAX_LEVELS} finite numbers")
    q = [quantise_scalar(v, scale if is_float else 1.0) for v in lv]
    for i in range(1, len(q)):
        if q[i] <= q[i - 1]:
            raise InsarError(f"{who}: levels must be strictly increasing after quantisation: levels[{i - 1}]={lv[i - 1]!r} -> "
                             f"{q[i - 1]}, levels[{i}]={lv[i]!r} -> {q[i]}")
    return np.asarray(q, dtype=np.int32)


def _check_args(raster, levels, scale, valid, nodata, max_vertices, max_lines):
    """Every refusal, none of which needs a device; those of host tensors come last. Returns (levels_q, has_nodata, nodata)."""
    who = "contour_lines"
    check_map(who, "raster", raster, tuple(_ELEM), of="the raster", one_fault=True)
    H, W = raster.shape
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise InsarError(f"{who}: raster {H} x {W}: need 1 <= H, W <= 2^22")
    try:
        scale_ok = math.isfinite(float(scale)) and float(scale) > 0
    except (TypeError, ValueError):
        scale_ok = False
    if not scale_ok:
        raise InsarError(f"{who}: scale={scale!r}: a positive finite number")
    levels_q = quantise_levels(levels, float(scale), raster.dtype == torch.float32)
    if len(levels_q) * H * W >= MAX_CELLS:
        raise InsarError(f"{who}: levels * H * W = {len(levels_q)} * {H} * {W} must stay below 2^30")
    if valid is not None:
        check_map(who, "valid", valid, (torch.uint8,), shape=(H, W), of="the raster")
    has_nodata, nd = 0, 0.0
    if nodata is not None:
        nd = float(nodata)
        if math.isnan(nd):
            raise InsarError(f"{who}: nodata is NaN: NaN pixels are invalid already, and nothing equals NaN")
        if raster.dtype != torch.float32:
            lo_t, hi_t = (0, 255) if raster.dtype == torch.uint8 else (-(1 << 31), (1 << 31) - 1)
            if nd != int(nd) or not lo_t <= int(nd) <= hi_t:
                raise InsarError(f"{who}: nodata={nodata!r} is no value of a {raster.dtype} raster")
        has_nodata = 1
    for name, v in (("max_vertices", max_vertices), ("max_lines", max_lines)):
        check_int(who, name, v, 1, 1 << 30, integral_floats=False)
    check_on_device(who, "raster", raster)
    if valid is not None:
        check_on_device(who, "valid", valid, like=raster)
    return levels_q, has_nodata, nd


def lines_from_table(raw: np.ndarray, n_lines: int) -> Dict[str, np.ndarray]:
    """The host line table (fresh arrays) from the raw bytes of a device table holding n_lines lines."""
    r = raw[HEADER_RECORDS * LINE_DTYPE.itemsize:].view(LINE_DTYPE)[:n_lines]
    out = {"line": np.arange(n_lines, dtype=np.int32)}
    for f in LINE_FIELDS[1:]:
        out[f] = r[f].astype(np.bool_) if f == "closed" else r[f].copy()
    return out


def _result(vertices, lines, level_counts, levels_q, scale, is_float) -> dict:
    return {"vertices": vertices, "lines": lines, "n_lines": int(len(lines["line"])), "n_vertices": int(vertices.shape[0]),
            "level_counts": level_counts, "levels_q": levels_q, "scale": float(scale) if is_float else 1.0}


def contour_lines(raster: torch.Tensor, levels, *, scale: float = 2 ** 16, valid: Optional[torch.Tensor] = None,
                  nodata: Optional[float] = None, max_vertices: int = DEFAULT_MAX_VERTICES, max_lines: int = DEFAULT_MAX_LINES,
                  scratch: Optional[ContourScratch] = None) -> dict:
    """The iso-lines of a device raster (float32, uint8 or int32 [H, W]) at `levels` (1..32 numbers in raster units).

        c = contour_lines(prob[1], [0.5])
        c["vertices"]      device int32 [V, 2] as (Y, X) in 1/256 pixel, line after line; the centre of pixel (y, x) is
                           (256 y + 128, 256 x + 128), in the frame of `region_outlines` times 256
        c["lines"]         dict of numpy arrays of length n_lines: line, level (index), closed, start, count (the line's slice of
                           the vertex array), leader (crossing id), area2 (int64 in 1/256^2 pixel; positive round a peak, negative
                           round a pit, 0 for open lines), y0, x0, y1, x1 (half-open box in 1/256 pixel)
        c["n_lines"], c["n_vertices"], c["level_counts"] (int64 [L], crossings per level), c["levels_q"] (int32 [L]), c["scale"]

    `scale` quantises a float32 raster and the levels (integer rasters are taken as they are); `valid` (uint8 [H, W], 0 = not
    observed), `nodata` (in the raster's own type) and non-finite pixels are invalid, and lines end beside them. 11 + 2
    ceil(log2 E) launches on the current stream and TWO device-to-host read-backs: the header with the crossing count E, which
    sizes the doubling rounds, then the header and the line table. More crossings than `max_vertices` or lines than `max_lines`
    raise InsarError. `scratch`: a ContourScratch of this raster size, level count and capacities to reuse (else allocated)."""
    levels_q, has_nodata, nd = _check_args(raster, levels, scale, valid, nodata, max_vertices, max_lines)
    H, W = raster.shape
    L, max_vertices, max_lines = len(levels_q), int(max_vertices), int(max_lines)
    key = (H, W, L, max_lines, max_vertices)
    if scratch is None:
        scratch = ContourScratch(H, W, raster.device, L, max_lines, max_vertices)
    else:
        ContourScratch.check("contour_lines", scratch, key, raster.device)
    is_float = raster.dtype == torch.float32
    lv = (C.c_int32 * L)(*levels_q.tolist())
    sp, tp = ptr(scratch.scratch), ptr(scratch.table)
    hdr_bytes = HEADER_RECORDS * LINE_DTYPE.itemsize
    with torch.cuda.device(raster.device):
        s = _lib.stream_ptr()
        call("insar_contour_edges", ptr(raster), _ELEM[raster.dtype], H, W, float(scale), has_nodata, nd, ptr(valid), lv, L,
             max_vertices, sp, tp, s)
        hdr = read_back(scratch.host, scratch.table, hdr_bytes).view(np.int32)
        E = int(hdr[HDR_CROSSINGS])
        level_counts = hdr[HDR_LEVELS:HDR_LEVELS + L].astype(np.int64)
        if E > max_vertices:
            raise InsarError(f"contour_lines: {E} vertices exceed max_vertices={max_vertices}: raise max_vertices or take fewer levels")
        vertices = torch.empty(E, 2, dtype=torch.int32, device=raster.device)
        if E == 0:
            return _result(vertices, lines_from_table(np.zeros(hdr_bytes, dtype=np.uint8), 0), level_counts, levels_q, scale, is_float)
        call("insar_contour_lead", H, W, L, E, max_vertices, sp, s)
        call("insar_contour_rank", H, W, L, E, max_vertices, sp, s)
        call("insar_contour_lines", H, W, L, E, max_lines, max_vertices, sp, tp, s)
        call("insar_contour_write", H, W, L, E, max_lines, max_vertices, sp, tp, ptr(vertices), s)
        # a line has two vertices or more: E / 2 bounds the records worth copying, whatever max_lines is
        raw = read_back(scratch.host, scratch.table, hdr_bytes + LINE_DTYPE.itemsize * min(max_lines, E // 2))
    n_lines = int(raw[:hdr_bytes].view(np.int32)[HDR_LINES])
    if n_lines > max_lines:
        raise InsarError(f"contour_lines: {n_lines} lines exceed max_lines={max_lines}: raise max_lines or take fewer levels")
    return _result(vertices, lines_from_table(raw, n_lines), level_counts, levels_q, scale, is_float)


# ---- simplification ------------------------------------------------------------------------------------------------------------
MAX_COORD = 1 << 30                      # the contract of simplify_contours: 0 <= Y, X <= 2^30 (contour_lines stays below it)
MAX_SIMPLIFY_VERTICES = 1 << 28
MAX_SIMPLIFY_LINES = 1 << 27
SIMPLIFIED_FIELDS = LINE_FIELDS + ("input_area2", "collapsed")
_NEEDED = ("level", "closed", "start", "count", "leader", "area2")


def contour_simplify_scratch_bytes(max_vertices: int, max_lines: int):
    """(scratch bytes, table bytes) of `simplify_contours` for these capacities. Host arithmetic only."""
    return query_bytes("insar_contour_simplify_scratch_bytes", max_vertices, max_lines, outputs=2)


def contour_simplify_launches(rounds: int) -> int:
    """Kernel launches of one `simplify_contours` call that issues `rounds` rounds (the probe after max_rounds counts as
    one): 12 + 5 rounds."""
    return call("insar_contour_simplify_launches", int(rounds))


def eps_q(tolerance: float) -> int:
    """round(256 * tolerance): the tolerance in 1/256 pixel, ties to even."""
    return int(round(float(tolerance) * SUBPIXEL))


class ContourSimplifyScratch(Scratch):
    """The device buffers of one (max_vertices, max_lines): scratch, the input and the output line table, and the pinned host
    copies of the tables and of one round counter. Nothing in them has to survive between calls or be cleared. The vertex and
    index arrays are the caller's: every call returns fresh ones."""
    KEY, DEVICE_AT = ("max_vertices", "max_lines"), 2

    def __init__(self, max_vertices: int, max_lines: int, device):
        sb, tb = contour_simplify_scratch_bytes(max_vertices, max_lines)
        super().__init__((max_vertices, max_lines), device, scratch=sb, table_in=tb, table=tb, host=tb)
        self.host_in, self.counter = pinned(tb), pinned(4)


def _check_simplify(contours, tolerance, max_rounds, scratch):
    """Everything `simplify_contours` refuses, none of which needs a device. Returns (vertices, lines, n_lines)."""
    who = "simplify_contours"
    if not isinstance(contours, dict) or "vertices" not in contours or "lines" not in contours:
        raise InsarError(f"{who}: contours must be a dict of the shape contour_lines returns, with 'vertices' and 'lines'")
    v, ln = contours["vertices"], contours["lines"]
    if not isinstance(v, torch.Tensor):
        raise InsarError(f"{who}: contours['vertices'] must be a torch tensor, got {type(v).__name__}")
    if v.dtype != torch.int32 or v.dim() != 2 or v.shape[1] != 2 or not v.is_contiguous():
        raise InsarError(f"{who}: contours['vertices'] must be a contiguous int32 tensor [V, 2], got {v.dtype} {tuple(v.shape)}")
    if not isinstance(ln, dict) or any(f not in ln for f in _NEEDED):
        raise InsarError(f"{who}: contours['lines'] must hold {', '.join(_NEEDED)}")
    R = len(ln["start"])
    if any(np.asarray(ln[f]).shape != (R,) for f in _NEEDED):
        raise InsarError(f"{who}: the fields of contours['lines'] differ in length")
    check_tolerance(who, "tolerance", tolerance)
    check_int(who, "max_rounds", max_rounds, 1, MAX_ROUNDS, integral_floats=False)
    V = int(v.shape[0])
    if V > MAX_SIMPLIFY_VERTICES or R > MAX_SIMPLIFY_LINES:
        raise InsarError(f"{who}: {V} vertices in {R} lines: at most 2^28 and 2^27")
    start, count = np.asarray(ln["start"], dtype=np.int64), np.asarray(ln["count"], dtype=np.int64)
    if (start != np.concatenate([[0], np.cumsum(count)[:-1]])).any() or int(count.sum()) != V:
        raise InsarError(f"{who}: the lines must tile the vertex array: start[0] = 0, start[i + 1] = start[i] + count[i], "
                         f"counts adding up to {V}")
    short = np.flatnonzero(count < np.where(np.asarray(ln["closed"], dtype=bool), 3, 2))
    if len(short):
        i = int(short[0])
        raise InsarError(f"{who}: line {i} is {'closed' if ln['closed'][i] else 'open'} and has {int(count[i])} "
                         f"vertices: an open line needs 2, a closed one 3")
    if scratch is not None:
        if not isinstance(scratch, ContourSimplifyScratch):
            raise InsarError(f"{who}: scratch must be a ContourSimplifyScratch, got {type(scratch).__name__}")
        if scratch.max_vertices < V or scratch.max_lines < R or scratch.device != v.device:
            raise InsarError(f"{who}: scratch for {scratch.max_vertices} vertices in {scratch.max_lines} lines on {scratch.device}: "
                             f"the input has {V} vertices in {R} lines on {v.device}")
    return v, ln, R


def _carried(contours: dict, out: dict) -> dict:
    for k in ("level_counts", "levels_q", "scale"):
        if k in contours:
            out[k] = contours[k]
    return out


def simplify_contours(contours: dict, *, tolerance: float, max_rounds: int = DEFAULT_MAX_ROUNDS,
                      scratch: Optional[ContourSimplifyScratch] = None) -> dict:
    """Douglas-Peucker simplification of the lines of `contours` (a dict of the shape `contour_lines` returns) on the device.

        c = contour_lines(smooth_raster(prob[1], gaussian_taps(1.5)), [0.5])
        s = simplify_contours(c, tolerance=0.5)
        s["vertices"]   device int32 [V', 2]: the kept vertices in input order, line after line
        s["kept"]       device int32 [V']: their positions in c["vertices"]
        s["lines"]      the line table of `contour_lines` with start / count in the compacted array, area2 (exact int64) and the
                        half-open box recomputed from the kept vertices; level, closed and leader unchanged; `input_area2`,
                        the input's area2 (its sign still tells a peak from a pit); `collapsed`: a ring with fewer than 3
                        kept vertices or area2 == 0 (an open line never collapses)
        s["n_lines"] (unchanged), ["n_vertices"] = V', ["input_n_vertices"], ["rounds"], ["converged"], and level_counts,
        levels_q, scale as they came

    Only the dict is read, no raster: hand-made polylines are valid input, with coordinates in 0 .. 2^30 (the contract: the
    host cannot check it without a read-back, and every overflow bound rests on it; `contour_lines` stays below it). Every
    line is simplified on its own. An open line keeps both ends; a ring starts from its smallest (Y, X) vertex and the vertex
    farthest from it. Every round keeps, in every segment between two kept vertices, the vertex farthest from the chord if it
    lies beyond `tolerance`, ties to the smallest (Y, X), then to the smallest position. `tolerance`: pixels, 0 .. 1024,
    quantised to 1/256; at 0 exactly the collinear vertices go. `max_rounds` (default 64, at most 4095) bounds the recursion
    depth: if some segment would still split after it, the result is the full result truncated at that depth and
    `converged` is False. Integers only: every output is bitwise reproducible (tests/contour_simplify_ref.py restates it).

    Guaranteed: every dropped vertex lies within `tolerance` of the chord of the segment it ended in; the ends of open lines
    stay; kept sets are nested over tolerances. Not guaranteed: lines of different levels, or two lines of one level, may
    cross at a large tolerance, and a hole may then fall outside its simplified exterior (`contour_polygons` raises as for any
    such input); `rasterise_polygons` of the polygons gives back {q >= level} bit for bit at tolerance 0 only.

    12 + 5 launches per round on the current stream; the host reads one 4-byte counter per 8 rounds to stop launching once
    a round kept nothing, then the line table once. `scratch`: a ContourSimplifyScratch with room for the input (else
    allocated). An empty input returns an empty result. `contours` is not written."""
    v, ln, R = _check_simplify(contours, tolerance, max_rounds, scratch)
    V = int(v.shape[0])
    if V == 0:
        lines = lines_from_table(np.zeros(HEADER_RECORDS * LINE_DTYPE.itemsize, dtype=np.uint8), 0)
        lines.update(input_area2=np.zeros(0, dtype=np.int64), collapsed=np.zeros(0, dtype=np.bool_))
        return _carried(contours, {"vertices": torch.empty(0, 2, dtype=torch.int32, device=v.device),
                                   "kept": torch.empty(0, dtype=torch.int32, device=v.device), "lines": lines, "n_lines": 0,
                                   "n_vertices": 0, "input_n_vertices": 0, "rounds": 0, "converged": True})
    check_on_device("simplify_contours", "vertices", v)
    if scratch is None:
        scratch = ContourSimplifyScratch(V, R, v.device)
    nbytes = LINE_DTYPE.itemsize * (1 + R)
    tin = scratch.host_in.numpy()[:nbytes].view(LINE_DTYPE)
    tin[:] = 0
    for f in ("level", "closed", "start", "count", "leader"):
        tin[f][1:] = ln[f]
    raw, out_v, out_k = simplify_rounds("insar_contour_simplify", scratch, v, R, nbytes, eps_q(tolerance) ** 2, int(max_rounds))
    raw = raw.view(LINE_DTYPE)
    head, rec = raw[0], raw[1:]
    kept = int(head["count"])
    lines = {"line": np.arange(R, dtype=np.int32)}
    for f in LINE_FIELDS[1:]:
        lines[f] = rec[f].astype(np.bool_) if f == "closed" else rec[f].copy()
    lines["input_area2"] = np.asarray(ln["area2"]).astype(np.int64)
    lines["collapsed"] = rec["_pad"] != 0
    return _carried(contours, {"vertices": out_v[:kept], "kept": out_k[:kept], "lines": lines, "n_lines": R, "n_vertices": kept,
                               "input_n_vertices": V, "rounds": int(head["leader"]), "converged": bool(head["start"])})


# ---- host side: coordinates, polygons, GeoJSON ------------------------------------------------------------------------------------
def _host_vertices(contours: dict) -> np.ndarray:
    v = contours["vertices"]
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _level_value(contours: dict, i: int) -> float:
    return float(contours["levels_q"][i]) / float(contours.get("scale", 1.0))


def _collapsed(contours: dict):
    """The `collapsed` flags of a simplified dict, None for a dict that `simplify_contours` did not make."""
    c = contours["lines"].get("collapsed")
    return None if c is None else np.asarray(c, dtype=bool)


def lines_to_coords(contours: dict, transform=None, drop_collapsed: bool = True) -> List[dict]:
    """One entry per line, in line order: {"level": index, "value": the level in raster units as it was quantised, "closed",
    "xy": float64 [n, 2]}. Without `transform` xy is (x, y) in pixels in the frame of `region_outlines` (vertex / 256, exact);
    with a 2 x 3 affine it is the world coordinate A @ (x, y, 1), the convention of `to_polygons`. Closed lines are not
    repeated at their end. Of a dict `simplify_contours` made, the collapsed rings are left out unless `drop_collapsed` is
    False; any other dict has none."""
    A = None
    if transform is not None:
        A = np.asarray(transform, dtype=np.float64)
        if A.shape != (2, 3):
            raise InsarError(f"transform must be a 2 x 3 affine, got shape {A.shape}")
    v = _host_vertices(contours).astype(np.float64) / SUBPIXEL
    ln = contours["lines"]
    gone = _collapsed(contours) if drop_collapsed else None
    out = []
    for i in range(len(ln["level"])):
        if gone is not None and gone[i]:
            continue
        s, n = int(ln["start"][i]), int(ln["count"][i])
        xy = v[s:s + n, ::-1]
        if A is not None:
            xy = np.concatenate([xy, np.ones((n, 1))], axis=1) @ A.T
        out.append({"level": int(ln["level"][i]), "value": _level_value(contours, int(ln["level"][i])),
                    "closed": bool(ln["closed"][i]), "xy": np.ascontiguousarray(xy)})
    return out


def contours_to_geojson(contours: dict, transform=None, drop_collapsed: bool = True) -> dict:
    """A GeoJSON FeatureCollection: one LineString feature per line with the properties "level" (index), "value" and "closed";
    coordinates are [x, y] lists as `lines_to_coords` gives them (`drop_collapsed` as there), and a closed line repeats its
    first point. json-serialisable types only."""
    feats = []
    for e in lines_to_coords(contours, transform, drop_collapsed):
        xy = e["xy"]
        if e["closed"]:
            xy = np.concatenate([xy, xy[:1]], axis=0)
        feats.append({"type": "Feature", "properties": {"level": e["level"], "value": e["value"], "closed": e["closed"]},
                      "geometry": {"type": "LineString", "coordinates": [[float(x), float(y)] for x, y in xy]}})
    return {"type": "FeatureCollection", "features": feats}


def _inside(ring: np.ndarray, py: int, px: int) -> bool:
    """Even-odd in integers: does the ray from (py, px) towards -x cross the ring (int64 [n, 2] as (Y, X)) an odd number of
    times? A segment counts iff it spans py half-openly (min <= py < max) and meets the ray's line left of px; the side is
    the sign of a cross product. The point must not lie on the ring."""
    a, b = ring, np.roll(ring, -1, axis=0)
    lo, hi = np.where((a[:, 0] <= b[:, 0])[:, None], a, b), np.where((a[:, 0] <= b[:, 0])[:, None], b, a)
    span = (lo[:, 0] <= py) & (py < hi[:, 0])
    # (px, py) lies right of the upward segment lo -> hi  <=>  the crossing lies left of px
    cross = (hi[:, 1] - lo[:, 1]) * (py - lo[:, 0]) - (px - lo[:, 1]) * (hi[:, 0] - lo[:, 0])
    return bool((span & (cross < 0)).sum() & 1)


def contour_polygons(contours: dict, level_index: int) -> List[dict]:
    """The set {q >= level} of one level as polygons, in the list form `to_polygons` returns: [{"label": 1, "polygons":
    [{"exterior": float64 [n, 2], "holes": [...]}, ...]}] (empty without a ring). Coordinates are (y, x) = vertex / 256, which is
    exact, rings closed by repeating the first vertex; `pack_polygons` takes them as they are. Rings of positive area2 are
    exteriors; every ring of negative area2 goes to the smallest-area exterior that contains its first vertex, by the even-odd
    rule in integers. A level with an open line is refused: its set is not bounded by rings alone. Of a dict
    `simplify_contours` made, exteriors and holes are told apart by the sign of `input_area2` (a simplified ring may turn
    over or lose its area), collapsed rings are skipped, and a collapsed exterior takes its holes with it: a hole that no
    remaining exterior contains is dropped where its level has a collapsed exterior, and refused as ever where it has none."""
    who = "contour_polygons"
    ln = contours["lines"]
    L = len(contours["levels_q"])
    level_index = check_int(who, "level_index", level_index, 0, L - 1, integral_floats=False)
    idx = np.flatnonzero(np.asarray(ln["level"]) == level_index)
    opened = [int(i) for i in idx if not ln["closed"][i]]
    if opened:
        raise InsarError(f"{who}: level {level_index} has {len(opened)} open line(s) (line {opened[0]} first): the set is bounded "
                         "by the raster border or by no-data there, not by rings")
    v = _host_vertices(contours).astype(np.int64)
    gone = _collapsed(contours)
    sign = ln["area2"] if gone is None else ln["input_area2"]
    lost_exterior = False
    if gone is not None:
        lost_exterior = any(gone[i] and sign[i] > 0 for i in idx)
        idx = [i for i in idx if not gone[i]]
    ring = {int(i): v[int(ln["start"][i]):int(ln["start"][i]) + int(ln["count"][i])] for i in idx}
    ext = [i for i in ring if sign[i] > 0]
    polys = {i: {"exterior": np.concatenate([ring[i], ring[i][:1]]) / float(SUBPIXEL), "holes": []} for i in ext}
    for i in ring:
        if sign[i] >= 0:
            continue
        py, px = int(ring[i][0, 0]), int(ring[i][0, 1])
        holding = [e for e in ext if ln["y0"][e] <= py < ln["y1"][e] and ln["x0"][e] <= px < ln["x1"][e] and _inside(ring[e], py, px)]
        if not holding and lost_exterior:
            continue
        if not holding:
            raise InsarError(f"{who}: no ring of positive area of level {level_index} contains line {i}")
        polys[min(holding, key=lambda e: abs(int(ln["area2"][e])))]["holes"].append(np.concatenate([ring[i], ring[i][:1]]) / float(SUBPIXEL))
    return [{"label": 1, "polygons": [polys[i] for i in ext]}] if ext else []
