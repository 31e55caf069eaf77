"""A sequential restatement of contour simplification (include/insar_hip.h, "contour simplification"): Douglas-Peucker over the
polylines of a `contour_lines` dict, open lines and closed rings, one recursion level per round, in Python integers only (the
coordinates reach 2^30, so cross^2 reaches 2^120 and no fixed-width type holds the keep test). It shares no code with
insar_unet_ca_amd/contours.py or csrc/contour_simplify.hip. The oracle of tests/test_contour_simplify_gpu.py, pinned by its
own invariants in tests/test_contour_simplify_host.py. Also the hand-made polylines both files use."""
import numpy as np

LINE_FIELDS = ("line", "level", "closed", "start", "count", "leader", "area2", "y0", "x0", "y1", "x1", "input_area2", "collapsed")
SUBPIXEL = 256
MASK64 = (1 << 64) - 1


def eps_of(tolerance):
    """round(256 * tolerance): the product is exact in binary floating point for the tolerances the tests use, Python's round
    takes ties to even."""
    return int(round(SUBPIXEL * float(tolerance)))


def exact(a, b):
    return a * b


def wrapped64(a, b):
    """The product as a kernel that multiplies in 64 bits would see it."""
    return (a * b) & MASK64


def seeds_of(pts, closed):
    """The local positions a line starts from: both ends of an open line; of a ring the position of the smallest (Y, X) and
    the one farthest from it (largest d^2, ties to the smallest (Y, X), then to the smallest position)."""
    n = len(pts)
    if not closed:
        return [0, n - 1]
    s1 = min(range(n), key=lambda i: (pts[i][0], pts[i][1], i))
    y1, x1 = pts[s1]
    s2 = min(range(n), key=lambda i: (-((pts[i][0] - y1) ** 2 + (pts[i][1] - x1) ** 2), pts[i][0], pts[i][1], i))
    return sorted({s1, s2})


def interior(a, b, n, closed):
    """The local positions strictly between a and b going forward; in a ring a >= b wraps, and a == b is all but a."""
    if b > a:
        return list(range(a + 1, b))
    assert closed
    return list(range(a + 1, n)) + list(range(0, b))


def winner_of(pts, idx, a, b, eps2, mul=exact):
    """The position among idx that a round keeps for the segment (a, b), or None. `mul` multiplies the two products of the
    keep test (exact, or wrapped to 64 bits to show what a narrow kernel would do)."""
    (ay, ax), (by, bx) = pts[a], pts[b]
    dy, dx = by - ay, bx - ax
    len2 = dy * dy + dx * dx
    best = None
    for p in idx:
        py, px = pts[p][0] - ay, pts[p][1] - ax
        m = abs(dx * py - dy * px) if len2 else py * py + px * px
        cand = (-m, pts[p][0], pts[p][1], p)
        if best is None or cand < best:
            best = cand
    if best is None:
        return None
    m = -best[0]
    beyond = mul(m, m) > mul(eps2, len2) if len2 else m > eps2
    return best[3] if beyond else None


def kept_of_line(pts, closed, eps2, max_rounds, mul=exact):
    """(sorted kept local positions, rounds that kept something, converged) of one line alone."""
    n = len(pts)
    kept = set(seeds_of(pts, closed))
    ks = sorted(kept)
    if closed:
        pending = [(ks[i], ks[(i + 1) % len(ks)]) for i in range(len(ks))]
    else:
        pending = [(ks[0], ks[1])]
    rounds, converged = 0, True
    for level in range(max_rounds + 1):                          # level max_rounds only probes
        nxt = []
        for a, b in pending:
            w = winner_of(pts, interior(a, b, n, closed), a, b, eps2, mul)
            if w is None:
                continue
            if level == max_rounds:
                converged = False
                break
            kept.add(w)
            nxt += [(a, w), (w, b)]
        if not nxt:
            break
        rounds += 1
        pending = nxt
    return sorted(kept), rounds, converged


def simplify_contours_oracle(contours, tolerance, max_rounds=64, mul=exact):
    """The dict `simplify_contours` returns, in numpy. Rounds are global: round r is recursion level r of every line, `rounds`
    the deepest level that kept a vertex anywhere, `converged` whether no line would split at level max_rounds."""
    v = [(int(y), int(x)) for y, x in np.asarray(contours["vertices"]).reshape(-1, 2)]
    ln = contours["lines"]
    eps2 = eps_of(tolerance) ** 2
    n_lines = len(ln["start"])
    kept_all, rounds, converged = [], 0, True
    out = {f: [] for f in LINE_FIELDS}
    for r in range(n_lines):
        s, n, closed = int(ln["start"][r]), int(ln["count"][r]), bool(ln["closed"][r])
        pts = v[s:s + n]
        ks, rd, cv = kept_of_line(pts, closed, eps2, max_rounds, mul)
        rounds, converged = max(rounds, rd), converged and cv
        c = [pts[k] for k in ks]
        m = len(c)
        area2 = sum(c[i][1] * c[(i + 1) % m][0] - c[(i + 1) % m][1] * c[i][0] for i in range(m)) if closed else 0
        vals = {"line": r, "level": int(ln["level"][r]), "closed": closed, "start": len(kept_all), "count": m,
                "leader": int(ln["leader"][r]), "area2": area2, "y0": min(y for y, _ in c), "x0": min(x for _, x in c),
                "y1": max(y for y, _ in c) + 1, "x1": max(x for _, x in c) + 1, "input_area2": int(ln["area2"][r]),
                "collapsed": closed and (m < 3 or area2 == 0)}
        for f in LINE_FIELDS:
            out[f].append(vals[f])
        kept_all += [s + k for k in ks]
    dt = {"area2": np.int64, "input_area2": np.int64, "closed": np.bool_, "collapsed": np.bool_}
    lines = {f: np.asarray(a, dtype=dt.get(f, np.int32)) for f, a in out.items()}
    res = {"vertices": np.asarray([v[i] for i in kept_all], dtype=np.int32).reshape(-1, 2),
           "kept": np.asarray(kept_all, dtype=np.int32), "lines": lines, "n_lines": n_lines, "n_vertices": len(kept_all),
           "input_n_vertices": len(v), "rounds": rounds, "converged": converged}
    for k in ("level_counts", "levels_q", "scale"):
        if k in contours:
            res[k] = contours[k]
    return res


# ---- rasters ---------------------------------------------------------------------------------------------------------------------
def raster_cases():
    """name -> (float32 raster, levels): `smooth_map` rasters of 48 x 64 and 33 x 130 with enough bumps for rings and for
    lines that leave through the border; two have a NaN hole in the middle, beside which more lines end."""
    from tests.contours_ref import smooth_map

    def sm(H, W, seed, hole=False):
        m = smooth_map(H, W, seed, bumps=24, smax=6.0)
        if hole:
            m[H // 2 - 3:H // 2 + 3, W // 2 - 5:W // 2 + 6] = np.nan
        return m
    three = [-15.0, 0.0, 15.0]
    return {"48x64, 3 levels": (sm(48, 64, 5), three), "48x64, 1 level": (sm(48, 64, 5), [5.0]),
            "33x130, 3 levels": (sm(33, 130, 5), three), "33x130 NaN hole, 3 levels": (sm(33, 130, 7, True), three),
            "48x64 NaN hole, 1 level": (sm(48, 64, 7, True), [5.0])}


# ---- hand-made polylines --------------------------------------------------------------------------------------------------------
def make_contours(parts):
    """A dict of the shape `contour_lines` returns from [(points [(Y, X), ...], closed), ...]: one level, leaders in order."""
    verts, tab = [], {f: [] for f in LINE_FIELDS[:11]}
    for r, (pts, closed) in enumerate(parts):
        pts = [(int(y), int(x)) for y, x in pts]
        n = len(pts)
        area2 = sum(pts[i][1] * pts[(i + 1) % n][0] - pts[(i + 1) % n][1] * pts[i][0] for i in range(n)) if closed else 0
        row = dict(line=r, level=0, closed=bool(closed), start=len(verts), count=n, leader=2 * r, area2=area2,
                   y0=min(y for y, _ in pts), x0=min(x for _, x in pts), y1=max(y for y, _ in pts) + 1,
                   x1=max(x for _, x in pts) + 1)
        for f in tab:
            tab[f].append(row[f])
        verts += pts
    dt = {"area2": np.int64, "closed": np.bool_}
    return {"vertices": np.asarray(verts, dtype=np.int32).reshape(-1, 2),
            "lines": {f: np.asarray(a, dtype=dt.get(f, np.int32)) for f, a in tab.items()}, "n_lines": len(parts),
            "n_vertices": len(verts), "level_counts": np.asarray([len(verts)], dtype=np.int64),
            "levels_q": np.asarray([0], dtype=np.int32), "scale": 1.0}


def zigzag(n, seed, y0=1000, x0=1000):
    """An open line of n vertices going right in steps of 64..256 with a wandering Y: nothing collinear but by chance."""
    rng = np.random.default_rng(seed)
    x = x0 + np.cumsum(rng.integers(64, 257, size=n))
    y = y0 + 40000 + np.cumsum(rng.integers(-200, 201, size=n)) + rng.integers(-300, 301, size=n)
    return list(zip(y.tolist(), x.tolist()))


def wobbly_ring(n, seed, cy=600000, cx=600000, radius=400000):
    """A closed ring of n vertices round (cy, cx): a circle with a seeded radial wobble, counter-clockwise in (x, y)."""
    rng = np.random.default_rng(seed)
    t = 2 * np.pi * np.arange(n) / n
    r = radius * (1 + 0.05 * np.sin(7 * t) + 0.02 * np.cos(31 * t)) + rng.integers(-150, 151, size=n)
    return list(zip(np.rint(cy + r * np.sin(t)).astype(np.int64).tolist(), np.rint(cx + r * np.cos(t)).astype(np.int64).tolist()))


SCAN_PASS_TOLERANCES = (0.25, 16)
_SCAN_PASS = {}


def scan_pass_lines():
    """A short open line (so that no line starts on a block border), a ring of 69 000 vertices and an open line of 600: 69 677
    positions, more than the 65 536 that one pass of the one-work-group carry and prefix scans takes, with the ring across that
    boundary. Built once."""
    if "lines" not in _SCAN_PASS:
        _SCAN_PASS["lines"] = make_contours([(zigzag(77, 3), False), (wobbly_ring(69000, 2), True), (zigzag(600, 5), False)])
    return _SCAN_PASS["lines"]


def scan_pass_ring_kept(ref):
    """(kept positions of the ring before position 65 536, at or after it) of an oracle result of `scan_pass_lines`."""
    s, n = int(ref["lines"]["start"][1]), int(ref["lines"]["count"][1])
    k = ref["kept"][s:s + n]
    return int((k < 65536).sum()), int((k >= 65536).sum())


def scan_pass_oracle(tolerance):
    """The oracle of `scan_pass_lines` at one of SCAN_PASS_TOLERANCES, computed once per process and not to be written."""
    if tolerance not in _SCAN_PASS:
        _SCAN_PASS[tolerance] = simplify_contours_oracle(scan_pass_lines(), tolerance, 64)
    return _SCAN_PASS[tolerance]


def shedding_arc(n=40, step_deg=60.0, rho=0.7, radius=1 << 28, centre=1 << 29):
    """An open convex arc, an inward spiral of n vertices that turns by step_deg and shrinks by rho from vertex to vertex: the
    farthest vertex from every chord to its inner end is the one next to the chord's outer end, so every level of the
    recursion sheds one vertex and the depth is n - 2 (tests assert that of the oracle)."""
    import math
    return [(int(round(centre + radius * rho ** k * math.sin(math.radians(step_deg * k)))),
             int(round(centre + radius * rho ** k * math.cos(math.radians(step_deg * k))))) for k in range(n)]


def wide_lines(seed=7):
    """Hand-made lines at the far end of the coordinate range 0 .. 2^30: an open line whose chord is about 2^25 long with
    deviations of about 2^8 (cross^2 and eps2 |b - a|^2 both pass 2^64 at a tolerance of a pixel), a ring round the whole
    square (|cross| towards 2^60, d^2 towards 2^61) and a short open line in the far corner."""
    rng = np.random.default_rng(seed)
    top = 1 << 30
    n = 257
    x = top - (1 << 25) + (np.arange(n) << 17)
    y = top - 4096 + rng.integers(-300, 301, size=n)
    line = list(zip(y.tolist(), x.tolist()))
    side = np.linspace(0, top, 33).astype(np.int64)[:-1]
    wob = lambda: rng.integers(0, 2000, size=len(side))
    ring = (list(zip(wob().tolist(), side.tolist())) + list(zip(side.tolist(), (top - wob()).tolist()))
            + list(zip((top - wob()).tolist(), (top - side).tolist())) + list(zip((top - side).tolist(), wob().tolist())))
    corner = [(top, top - 5000), (top - 700, top - 2500), (top, top)]
    return [(line, False), (ring, True), (corner, False)]
