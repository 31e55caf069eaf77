"""A sequential restatement of the outline-simplification semantics (include/insar_hip.h, "outline simplification"): anchors
from the label map, the two seeds of a closed arc, level-synchronous Douglas-Peucker with the tie rule by coordinate, the
truncation at `max_rounds`, and the recomputed ring table; ring by ring and segment by segment, with numpy int64 for the
cross products (cross^2 < 2^60) and Python integers for the one comparison that would leave 64 bits. No GPU. The oracle of
tests/test_simplify_gpu.py, pinned by its own invariants in tests/test_simplify_host.py. Also the maps both files use."""
import numpy as np

RING_FIELDS = ("ring", "label", "start", "count", "edges", "area2", "hole", "y0", "x0", "y1", "x1", "leader", "collapsed")


def eps2q_of(tolerance):
    """round(tolerance * 16)^2: the product is exact in binary floating point, Python's round takes ties to even."""
    return int(round(float(tolerance) * 16)) ** 2


def anchor_mask(vertices, labels):
    """bool per vertex: three or more distinct values among its four pixels, or a two-label saddle without background."""
    v = np.asarray(vertices, dtype=np.int64).reshape(-1, 2)
    if labels is None:
        return np.zeros(len(v), dtype=bool)
    lab = np.asarray(labels)
    H, W = lab.shape
    pad = np.zeros((H + 2, W + 2), dtype=np.int64)
    pad[1:-1, 1:-1] = lab
    y, x = v[:, 0], v[:, 1]
    p00, p01, p10, p11 = pad[y, x], pad[y, x + 1], pad[y + 1, x], pad[y + 1, x + 1]     # pad[j + 1, i + 1] is pixel (j, i)
    distinct = 1 + (p01 != p00) + ((p10 != p00) & (p10 != p01)) + ((p11 != p00) & (p11 != p01) & (p11 != p10))
    saddle = (p00 == p11) & (p01 == p10) & (p00 != p01) & (p00 != 0) & (p01 != 0)
    return (distinct >= 3) | saddle


def _key(c):
    return c[:, 0] * 65536 + c[:, 1]


def seeds_of(c, anchors):
    """The positions a closed arc starts from: every position with the coordinates of seed 1 or seed 2 ([] with two anchors
    or more). c: int64 [n, 2] of one ring, anchors: bool [n]."""
    if anchors.sum() >= 2:
        return np.zeros(0, dtype=np.int64)
    key = _key(c)
    s1 = key[np.flatnonzero(anchors)[0]] if anchors.any() else key.min()
    d2 = (c[:, 0] - s1 // 65536) ** 2 + (c[:, 1] - s1 % 65536) ** 2
    s2 = key[d2 == d2.max()].min()
    return np.flatnonzero((key == s1) | (key == s2))


def _between(a, b, n):
    """The positions strictly between a and b going forward round a ring of n; a == b is the whole ring but a."""
    if b > a:
        return np.arange(a + 1, b, dtype=np.int64)
    return np.concatenate([np.arange(a + 1, n, dtype=np.int64), np.arange(0, b, dtype=np.int64)])


def winners_of(c, a, b, eps2q):
    """The positions of segment (a, b) of ring c that a round keeps (ascending along the segment), [] if none."""
    idx = _between(a, b, len(c))
    if len(idx) == 0:
        return idx
    d = c[b] - c[a]
    p = c[idx] - c[a]
    len2 = int(d[0] * d[0] + d[1] * d[1])
    if len2:
        cross = d[1] * p[:, 0] - d[0] * p[:, 1]
        num = cross * cross
    else:                                                        # the chord is a point: distance from the point
        num, len2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1], 1
    m = int(num.max())
    if not 256 * m > eps2q * len2:                               # Python integers: exact
        return idx[:0]
    key = _key(c[idx])
    best = key[num == m].min()
    return idx[(num == m) & (key == best)]


def simplify_oracle(vertices, rings, labels, tolerance, max_rounds):
    """The dict `simplify_outlines` returns, in numpy: vertices int32 [V', 2], kept int32 [V'], rings (RING_FIELDS),
    vertex_count, ring_count, edge_count, input_vertex_count, rounds, converged. `rings` needs start, count and whatever is
    copied (ring, label, edges, leader, area2)."""
    v = np.asarray(vertices, dtype=np.int64).reshape(-1, 2)
    eps2q = eps2q_of(tolerance)
    R = len(rings["start"])
    anchors = anchor_mask(v, labels)
    kept = anchors.copy()
    pending = []                                                 # (ring, a, b) in ring-local positions, still to examine
    for r in range(R):
        s, n = int(rings["start"][r]), int(rings["count"][r])
        loc = kept[s:s + n]
        loc[seeds_of(v[s:s + n], anchors[s:s + n])] = True
        ks = np.flatnonzero(loc)
        pending += [(r, int(ks[i]), int(ks[(i + 1) % len(ks)])) for i in range(len(ks))]
    rounds, converged = 0, True
    for level in range(max_rounds + 1):                          # level max_rounds only probes
        nxt = []
        for r, a, b in pending:
            s, n = int(rings["start"][r]), int(rings["count"][r])
            w = winners_of(v[s:s + n], a, b, eps2q)
            if len(w) == 0:
                continue
            if level == max_rounds:
                converged = False
                break
            kept[s + w] = True
            cut = [a] + [int(i) for i in w] + [b]
            nxt += [(r, cut[i], cut[i + 1]) for i in range(len(cut) - 1)]
        if not nxt:
            break
        rounds += 1
        pending = nxt
    idx = np.flatnonzero(kept)
    pos = np.concatenate([[0], np.cumsum(kept)])
    out = {f: [] for f in RING_FIELDS}
    for r in range(R):
        s, n = int(rings["start"][r]), int(rings["count"][r])
        c = v[s:s + n][kept[s:s + n]]
        m = len(c)
        area2 = sum(int(c[i, 1]) * int(c[(i + 1) % m, 0]) - int(c[(i + 1) % m, 1]) * int(c[i, 0]) for i in range(m))
        vals = {"ring": r, "label": rings["label"][r], "start": pos[s], "count": m, "edges": rings["edges"][r], "area2": area2,
                "hole": rings["area2"][r] < 0, "y0": c[:, 0].min(), "x0": c[:, 1].min(), "y1": c[:, 0].max() + 1,
                "x1": c[:, 1].max() + 1, "leader": rings["leader"][r], "collapsed": m < 3 or area2 == 0}
        for f in RING_FIELDS:
            out[f].append(vals[f])
    dt = {"area2": np.int64, "hole": np.bool_, "collapsed": np.bool_}
    out = {f: np.asarray(a, dtype=dt.get(f, np.int32)) for f, a in out.items()}
    return {"vertices": v[idx].astype(np.int32).reshape(-1, 2), "kept": idx.astype(np.int32), "rings": out,
            "vertex_count": len(idx), "ring_count": R, "edge_count": int(np.asarray(rings["edges"], dtype=np.int64).sum()),
            "input_vertex_count": len(v), "rounds": rounds, "converged": converged}


# ---- maps ----------------------------------------------------------------------------------------------------------------------
def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % 2 == 0).astype(np.int32)


def spiral(n):
    """A one-pixel-wide spiral path: walk inwards, turning right two cells before the path already laid."""
    m = np.zeros((n, n), dtype=np.int32)
    y, x, d, turns = 0, 0, 0, 0
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    m[0, 0] = 1
    while turns < 2:
        dy, dx = step[d]
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < n and 0 <= nx < n and m[ny, nx] == 0 and not (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def disc(radius=40, size=96):
    y, x = np.mgrid[:size, :size]
    return (((y - size // 2) ** 2 + (x - size // 2) ** 2) <= radius * radius).astype(np.int32) * 3


def ring_with_island():
    m = np.zeros((40, 46), dtype=np.int32)
    y, x = np.mgrid[:40, :46]
    d2 = (y - 20) ** 2 + (x - 23) ** 2
    m[d2 <= 18 * 18] = 4
    m[d2 <= 11 * 11] = 0
    m[d2 <= 5 * 5] = 4                                           # the same label inside its own hole
    return m


def two_label_staircase():
    """Label 1 left of a staircase border, label 2 right of it, and an island of 2 that directly fills a hole of 1."""
    m = np.zeros((30, 44), dtype=np.int32)
    for y in range(2, 28):
        cut = 12 + (y - 2) * 3 // 4 + (y % 3 == 0)
        m[y, 2:cut] = 1
        m[y, cut:42] = 2
    m[10:17, 4:9] = 2
    m[12, 8] = 1
    m[17, 5] = 2
    return m


def three_labels():
    """Three labels with T-junctions on straight sides, a two-label saddle, a three-label corner and an island of 3 that
    fills a hole of 1. Every region is one 8-connected component."""
    m = np.zeros((36, 48), dtype=np.int32)
    m[2:34, 2:20] = 1
    m[2:18, 20:46] = 2
    m[18:34, 20:46] = 3                                          # T-junctions at (18, 20), (2, 20), (34, 20), (18, 46)
    for k in range(7):                                           # a staircase between 2 and 3
        m[18 + k, 30 + 2 * k:46] = 2
    m[8:15, 6:13] = 3                                            # the island of 3 in 1
    m[10, 12] = 1
    m[24:26, 17:20] = 3                                          # 3 reaches into 1 ...
    m[26, 16] = 3                                                # ... and ends in a saddle with 1 at vertex (26, 17)
    return m


def blobs(H=96, W=160, seed=5, labels=4):
    """A seeded random map of smooth blobs: box-filtered noise cut into `labels` levels, 0 included."""
    rng = np.random.default_rng(seed)
    f = rng.random((H + 8, W + 8))
    c = np.cumsum(np.cumsum(np.pad(f, ((1, 0), (1, 0))), axis=0), axis=1)
    box = c[9:, 9:] - c[:-9, 9:] - c[9:, :-9] + c[:-9, :-9]
    q = np.quantile(box, np.linspace(0, 1, labels + 1)[1:-1])
    return np.digitize(box, q).astype(np.int32)[:H, :W]


def _lattice_ring(corners):
    """Every lattice vertex along the closed axis-parallel path through `corners`, as int32 [n, 2]."""
    pts = []
    for (y0, x0), (y1, x1) in zip(corners, corners[1:] + corners[:1]):
        n = max(abs(y1 - y0), abs(x1 - x0))
        pts += [(y0 + (y1 - y0) * k // n, x0 + (x1 - x0) * k // n) for k in range(n)]
    return np.asarray(pts, dtype=np.int32)


def circle_rings(radii):
    """Hand-made rings, not traced from a map: the pixel-edge outline of a disc per radius, all about one centre, every
    lattice vertex written (count == edges, about 8 r vertices each), as (vertices int32 [V, 2], rings dict). Their length
    is what the test wants it to be, which no map of a testable size gives."""
    c = max(radii)
    parts, rings = [], {f: [] for f in ("ring", "label", "start", "count", "edges", "area2", "hole", "y0", "x0", "y1", "x1", "leader")}
    at = 0
    for k, r in enumerate(radii):
        half = [int(np.sqrt(r * r - (j + 0.5 - r) ** 2)) for j in range(2 * r)]
        right, left = [], []
        for j, w in enumerate(half):                             # down the right flank, up the left one
            right += [(c - r + j, c + w), (c - r + j + 1, c + w)]
            left += [(c - r + j, c - w), (c - r + j + 1, c - w)]
        corners = right + left[::-1]
        corners = [p for i, p in enumerate(corners) if p != corners[i - 1]]
        v = _lattice_ring(corners)
        n = len(v)
        y, x = v[:, 0].astype(np.int64), v[:, 1].astype(np.int64)
        area2 = int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
        for f, val in (("ring", k), ("label", k + 1), ("start", at), ("count", n), ("edges", n), ("area2", area2), ("hole", area2 < 0),
                       ("y0", y.min()), ("x0", x.min()), ("y1", y.max() + 1), ("x1", x.max() + 1), ("leader", 4 * k)):
            rings[f].append(val)
        parts.append(v)
        at += n
    dt = {"area2": np.int64, "hole": np.bool_}
    return np.concatenate(parts), {f: np.asarray(a, dtype=dt.get(f, np.int32)) for f, a in rings.items()}
