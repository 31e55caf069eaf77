"""Outline simplification: Douglas-Peucker over the rings `region_outlines` traced, on the device, in exact integers, with the
common border of two regions simplified to the same vertices from both sides (csrc/simplify.hip: insar_simplify_setup /
_rounds / _finish). The result has the shape of the `region_outlines` dict, so `to_polygons`, `to_geojson` and `perimeters`
take it unchanged. `ScenePredictor.detect(..., outlines=True, simplify=1.0)` simplifies what it traced.

Semantics (include/insar_hip.h, "outline simplification"; tests/simplify_ref.py restates them sequentially): with the label
map, vertices where three labels meet (or two in a saddle) are anchors; they are always kept and cut every ring into arcs
that both neighbours see alike. A ring with fewer than two anchors starts from two seeds, its smallest (y, x) vertex (or its
anchor) and the vertex farthest from it. Every round keeps, in every segment between two kept vertices, the vertex farthest
from the chord if it lies beyond `tolerance`, ties to the smallest (y, x), never to the smallest index, so that both
directions of a shared arc agree. Integers only: every output is bitwise reproducible.

Guaranteed: every dropped vertex lies within `tolerance` of the chord of the segment it ended in; the kept set of a larger
tolerance is a subset of that of a smaller one; a shared arc is identical from both sides. Not guaranteed: that two different
arcs never cross at a large tolerance. Douglas-Peucker does not give that, and nothing here adds it.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import InsarError, call, ptr
from ._scene import MAX_TOLERANCE, ROUNDS_PER_READ  # noqa: F401  (the tools read them from here)
from ._scene import (DEFAULT_MAX_ROUNDS, MAX_ROUNDS, Scratch, check_int, check_map, check_on_device, check_tolerance, pinned,
                     query_bytes, simplify_rounds)
from .outlines import RING_DTYPE

MAX_DIM = 16384                          # the cap rasterise.py uses: cross^2 of two such vectors fits 64 bits
MAX_VERTICES = 1 << 28
MAX_RINGS = 1 << 26
_COPIED = ("label", "edges", "leader", "area2")


def scratch_bytes(max_vertices: int, max_rings: int):
    """(scratch bytes, table bytes) for these capacities. Host arithmetic only."""
    return query_bytes("insar_simplify_scratch_bytes", max_vertices, max_rings, outputs=2)


def launches(rounds: int) -> int:
    """Kernel launches of one call that issues `rounds` rounds (the probe after max_rounds counts as one): 10 + 4 rounds."""
    return call("insar_simplify_launches", int(rounds))


def eps2q(tolerance: float) -> int:
    """round(tolerance * 16)^2: the tolerance in 1/16 pixel, ties to even, squared."""
    return int(round(float(tolerance) * 16)) ** 2


class SimplifyScratch(Scratch):
    """The device buffers of one (max_vertices, max_rings, H, W): scratch, the input and the output ring table, and the pinned
    host copies of the tables and of one round counter. Nothing in them has to survive between calls. The vertex and index
    arrays are the caller's: every call returns fresh ones. H and W only name the scene the scratch serves."""
    KEY, DEVICE_AT = ("max_vertices", "max_rings", "H", "W"), 4

    def __init__(self, max_vertices: int, max_rings: int, H: int, W: int, device):
        sb, tb = scratch_bytes(max_vertices, max_rings)
        super().__init__((max_vertices, max_rings, H, W), device, scratch=sb, table_in=tb, table=tb, host=tb)
        self.host_in, self.counter = pinned(tb), pinned(4)


def _empty(device, outlines: dict) -> dict:
    rings = {f: np.zeros(0, dtype=np.int64 if f == "area2" else np.bool_ if f in ("hole", "collapsed") else np.int32)
             for f in ("ring", "label", "start", "count", "edges", "area2", "hole", "y0", "x0", "y1", "x1", "leader", "collapsed")}
    return {"vertices": torch.empty(0, 2, dtype=torch.int32, device=device), "kept": torch.empty(0, dtype=torch.int32, device=device),
            "rings": rings, "ring_count": 0, "vertex_count": 0, "edge_count": int(outlines.get("edge_count", 0)),
            "input_vertex_count": 0, "rounds": 0, "converged": True}


def _check_args(outlines, labels, tolerance, max_rounds):
    """Everything that can be refused without the device. Returns (vertices, rings, R, H, W)."""
    who = "simplify_outlines"
    if not isinstance(outlines, dict) or "vertices" not in outlines or "rings" not in outlines:
        raise InsarError(f"{who}: outlines must be the dict region_outlines returns, with 'vertices' and 'rings'")
    v, rings = outlines["vertices"], outlines["rings"]
    if not isinstance(v, torch.Tensor):
        raise InsarError(f"{who}: outlines['vertices'] must be a torch tensor, got {type(v).__name__}")
    if v.dtype != torch.int32 or v.dim() != 2 or v.shape[1] != 2 or not v.is_contiguous():
        raise InsarError(f"{who}: outlines['vertices'] must be a contiguous int32 tensor [V, 2], got {v.dtype} {tuple(v.shape)}")
    if not isinstance(rings, dict) or any(f not in rings for f in ("start", "count") + _COPIED):
        raise InsarError(f"{who}: outlines['rings'] must hold start, count, {', '.join(_COPIED)}")
    R = len(rings["start"])
    if any(len(np.asarray(rings[f])) != R for f in ("count",) + _COPIED):
        raise InsarError(f"{who}: the fields of outlines['rings'] differ in length")
    check_tolerance(who, "tolerance", tolerance)
    check_int(who, "max_rounds", max_rounds, 1, MAX_ROUNDS, integral_floats=False)
    H = W = 0
    if labels is not None:
        check_map(who, "labels", labels, (torch.int32,))
        H, W = labels.shape
        if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
            raise InsarError(f"{who}: label map {H} x {W}: 1 <= H, W <= {MAX_DIM}")
        if labels.device != v.device:
            raise InsarError(f"{who}: labels on {labels.device}, vertices on {v.device}")
    V = int(v.shape[0])
    if V > MAX_VERTICES or R > MAX_RINGS:
        raise InsarError(f"{who}: {V} vertices in {R} rings: at most 2^28 and 2^26")
    start, count = np.asarray(rings["start"], dtype=np.int64), np.asarray(rings["count"], dtype=np.int64)
    if (count < 1).any() or (start != np.concatenate([[0], np.cumsum(count)[:-1]])).any() or int(count.sum()) != V:
        raise InsarError(f"{who}: the rings must tile the vertex array: start[0] = 0, start[r + 1] = start[r] + count[r], "
                         f"counts adding up to {V}")
    if R and all(f in rings for f in ("y0", "x0", "y1", "x1")):
        hi_y, hi_x = (H, W) if labels is not None else (MAX_DIM, MAX_DIM)
        y0, x0 = int(np.min(rings["y0"])), int(np.min(rings["x0"]))
        y1, x1 = int(np.max(rings["y1"])) - 1, int(np.max(rings["x1"])) - 1
        if y0 < 0 or x0 < 0 or y1 > hi_y or x1 > hi_x:
            raise InsarError(f"{who}: the ring boxes span vertices ({y0}, {x0}) .. ({y1}, {x1}), outside "
                             + (f"the {H} x {W} label map" if labels is not None else f"0 .. {MAX_DIM}"))
    if labels is not None and (count != np.asarray(rings["edges"], dtype=np.int64)).any():
        bad = int(np.flatnonzero(count != np.asarray(rings["edges"]))[0])
        raise InsarError(f"{who}: with labels every ring needs count == edges (trace with corners_only=False): ring {bad} has "
                         f"{int(count[bad])} vertices on {int(rings['edges'][bad])} edges")
    return v, rings, R, int(H), int(W)


def simplify_outlines(outlines: dict, labels: Optional[torch.Tensor] = None, *, tolerance: float,
                      max_rounds: int = DEFAULT_MAX_ROUNDS, scratch: Optional[SimplifyScratch] = None) -> dict:
    """Douglas-Peucker simplification of the rings of `outlines` (the dict `region_outlines` returns) on the device.

        raw = region_outlines(det["labels"], corners_only=False)
        out = simplify_outlines(raw, det["labels"], tolerance=1.0)
        out["vertices"]  device int32 [V', 2]: the kept vertices in input order, ring after ring
        out["kept"]      device int32 [V']: their indices in raw["vertices"]
        out["rings"]     the ring table of `region_outlines` with start / count in the compacted array, area2 (exact int64) and
                         the box recomputed from the kept vertices, `hole` still from the input's area2, edges and leader
                         unchanged, and `collapsed`: fewer than 3 kept vertices or area2 == 0
        out["vertex_count"], ["ring_count"], ["edge_count"], ["input_vertex_count"], ["rounds"], ["converged"]

    `labels` (device int32 [H, W], H, W <= 16384, the map the rings were traced from) makes the result aware of shared
    borders: the common arc of two rings keeps the same vertices in both, so `rasterise_polygons` of the result reports no
    overlap at tolerance 0. It needs rings traced with corners_only=False. Without `labels` every ring is simplified on its
    own and either tracing mode is accepted. `tolerance`: pixels, 0 .. 1024, quantised to 1/16; at 0 only collinear vertices
    go. `max_rounds` (default 64, at most 4095) bounds the recursion depth: if some segment would still split after it, the
    result is the full result truncated at that depth and `converged` is False.

    Guaranteed: every dropped vertex lies within `tolerance` of the chord of the segment it ended in; kept sets are nested
    over tolerances; shared arcs are identical from both sides. Not guaranteed: that two different arcs never cross at a
    large tolerance.

    10 + 4 launches per round on the current stream; the host reads one 4-byte counter per 8 rounds to stop launching once
    a round kept nothing, then the ring table once. `scratch`: a SimplifyScratch with room for the input (else allocated).
    An empty input returns an empty result. Neither `outlines` nor `labels` is written."""
    v, rings, R, H, W = _check_args(outlines, labels, tolerance, max_rounds)
    V = int(v.shape[0])
    if V == 0:
        return _empty(v.device, outlines)
    check_on_device("simplify_outlines", "vertices", v)
    if scratch is None:
        scratch = SimplifyScratch(V, R, H, W, v.device)
    elif scratch.max_vertices < V or scratch.max_rings < R or scratch.scratch.device != v.device \
            or (labels is not None and (scratch.H, scratch.W) != (H, W)):
        raise InsarError(f"simplify_outlines: scratch for {scratch.max_vertices} vertices, {scratch.max_rings} rings of a "
                         f"{scratch.H} x {scratch.W} scene on {scratch.scratch.device}: the input has {V} vertices, {R} rings"
                         + (f" of a {H} x {W} scene" if labels is not None else "") + f" on {v.device}")
    nbytes = RING_DTYPE.itemsize * (1 + R)
    tin = scratch.host_in.numpy()[:nbytes].view(RING_DTYPE)
    tin[:] = 0
    tin["start"][1:], tin["count"][1:] = rings["start"], rings["count"]
    for f in _COPIED:
        tin[f][1:] = rings[f]
    raw, out_v, out_k = simplify_rounds("insar_simplify", scratch, v, R, nbytes, eps2q(tolerance), int(max_rounds), (ptr(labels), H, W))
    raw = raw.view(RING_DTYPE)
    head, rec = raw[0], raw[1:]
    kept = int(head["count"])
    out = {"ring": np.arange(R, dtype=np.int32)}
    for f in ("label", "start", "count", "edges", "area2", "y0", "x0", "y1", "x1", "leader"):
        out[f] = rec[f].copy()
    out["hole"] = np.asarray(rings["area2"]) < 0
    out["collapsed"] = rec["_pad"] != 0
    return {"vertices": out_v[:kept], "kept": out_k[:kept], "rings": out, "ring_count": R, "vertex_count": kept,
            "edge_count": int(outlines["edge_count"]) if "edge_count" in outlines else int(np.asarray(rings["edges"], dtype=np.int64).sum()),
            "input_vertex_count": V, "rounds": int(head["leader"]), "converged": bool(head["start"])}
