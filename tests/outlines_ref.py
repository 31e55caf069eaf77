"""A sequential restatement of the region-outline semantics (include/insar_hip.h, "region outlines"): boundary edges of a
label map, the successor rule, rings, area2, boxes and corner compaction, one edge at a time in Python; and an even-odd
rasteriser that takes rings back to a boolean map. The oracle of tests/test_outlines_gpu.py, pinned by its own invariants in
tests/test_outlines_host.py."""
import numpy as np

# travel direction of side s (0 top: east, 1 right: south, 2 bottom: west, 3 left: north) as (dy, dx)
DIRS = ((0, 1), (1, 0), (0, -1), (-1, 0))
RING_FIELDS = ("ring", "label", "start", "count", "edges", "area2", "hole", "y0", "x0", "y1", "x1")


def _at(labels, y, x):
    H, W = labels.shape
    return int(labels[y, x]) if 0 <= y < H and 0 <= x < W else 0


def boundary_edges(labels):
    """Edge ids 4 * (y * W + x) + s in ascending order."""
    H, W = labels.shape
    ids = []
    for y in range(H):
        for x in range(W):
            c = int(labels[y, x])
            if c == 0:
                continue
            for s, (ny, nx) in enumerate(((-1, 0), (0, 1), (1, 0), (0, -1))):
                if _at(labels, y + ny, x + nx) != c:
                    ids.append(4 * (y * W + x) + s)
    return ids


def successor(labels, eid, connectivity):
    H, W = labels.shape
    p, s = divmod(eid, 4)
    y, x = divmod(p, W)
    c = int(labels[y, x])
    dy, dx = DIRS[s]
    ay, ax = y + dy, x + dx
    ny, nx = DIRS[(s + 3) % 4]                      # the outer side of an edge lies towards d((s + 3) % 4)
    by, bx = ay + ny, ax + nx
    a, b = _at(labels, ay, ax) == c, _at(labels, by, bx) == c
    if a and b or (b and not a and connectivity == 8):
        return 4 * (by * W + bx) + (s + 3) % 4
    if a:
        return 4 * (ay * W + ax) + s
    return 4 * p + (s + 1) % 4


def tail_vertex(eid, W):
    p, s = divmod(eid, 4)
    y, x = divmod(p, W)
    return ((y, x), (y, x + 1), (y + 1, x + 1), (y + 1, x))[s]


def outlines_oracle(labels, connectivity=8, corners_only=True):
    """{"vertices": int32 [V, 2], "rings": dict of arrays (RING_FIELDS + "leader"), "ring_count", "vertex_count", "edge_count",
    "succ": {edge id: edge id}}"""
    labels = np.asarray(labels)
    H, W = labels.shape
    ids = boundary_edges(labels)
    succ = {e: successor(labels, e, connectivity) for e in ids}
    seen = set()
    rings = {f: [] for f in RING_FIELDS + ("leader",)}
    verts = []
    for lead in ids:                                 # ascending: the first unseen edge of a ring is its smallest
        if lead in seen:
            continue
        cyc, e = [], lead
        while e not in seen:
            seen.add(e)
            cyc.append(e)
            e = succ[e]
        assert e == lead, "the successor map is not a permutation"
        tails = [tail_vertex(e, W) for e in cyc]
        n = len(cyc)
        area2 = sum(tails[i][1] * tails[(i + 1) % n][0] - tails[(i + 1) % n][1] * tails[i][0] for i in range(n))
        keep = [tails[i] for i in range(n) if not corners_only or cyc[i] % 4 != cyc[i - 1] % 4]
        ys, xs = [t[0] for t in tails], [t[1] for t in tails]
        for f, v in (("ring", len(rings["ring"])), ("label", int(labels.flat[lead // 4])), ("leader", lead), ("start", len(verts)),
                     ("count", len(keep)), ("edges", n), ("area2", area2), ("hole", area2 < 0), ("y0", min(ys)), ("x0", min(xs)),
                     ("y1", max(ys) + 1), ("x1", max(xs) + 1)):
            rings[f].append(v)
        verts.extend(keep)
    dt = {"area2": np.int64, "hole": np.bool_}
    rings = {f: np.asarray(v, dtype=dt.get(f, np.int32)) for f, v in rings.items()}
    vertices = np.asarray(verts, dtype=np.int32).reshape(-1, 2)
    return {"vertices": vertices, "rings": rings, "ring_count": len(rings["ring"]), "vertex_count": len(vertices),
            "edge_count": len(ids), "succ": succ}


def rasterise(rings_yx, H, W):
    """Even-odd fill of closed rectilinear rings (arrays [n, 2] of lattice vertices (y, x), closed or not): pixel (y, x) is
    inside iff a ray from its centre towards -x crosses an odd number of vertical ring segments."""
    cross = np.zeros((H, W + 1), dtype=np.int64)
    for ring in rings_yx:
        r = np.asarray(ring).reshape(-1, 2)
        n = len(r)
        for i in range(n):
            (y0, x0), (y1, x1) = r[i], r[(i + 1) % n]
            if x0 == x1 and y0 != y1:
                cross[min(y0, y1):max(y0, y1), x0] += 1
    return (np.cumsum(cross, axis=1)[:, :W] % 2).astype(bool)


def perimeter_by_label(rings):
    out = {}
    for lab, e in zip(rings["label"].tolist(), rings["edges"].tolist()):
        out[lab] = out.get(lab, 0) + e
    return out
