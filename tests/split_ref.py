"""Sequential numpy restatement of insar_unet_ca_amd.split.split_regions, written from the rule ("Splitting
touching sites"), not from the kernels: ascent along the total order key(p) = (h[p], -index(p)), saddles between basins of one
label, synchronous merge rounds, numbering by smallest pixel index. Heights come from tests/distance_ref.py, so no test needs
scipy. A helper, not a test module; tests/test_split_host.py pins it on the prototype cases."""
import math

import numpy as np

from . import distance_ref as dr

CONF_SCALE = 1 << 30
FAR = dr.FAR
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def heights_oracle(labels, max_distance=None):
    """int32 [H, W]: d2 of the "edge" transform of the label map; with a bound R the far value is R * R."""
    labels = np.asarray(labels, dtype=np.int32)
    d2 = dr.cap(dr.dist_oracle(dr.sites_oracle(labels, "edge", None)), max_distance)
    if max_distance is not None:
        d2 = np.where(d2 == FAR, np.int32(int(max_distance) ** 2), d2).astype(np.int32)
    return d2


def threshold(min_depth, squared):
    """T of the merge rule: sixteenths of a pixel in squared mode (rint: half to even), the number itself in linear mode."""
    return int(np.rint(float(min_depth) * 16.0)) if squared else int(min_depth)


def depth(P, S, squared):
    P, S = int(P), int(S)
    return math.isqrt(256 * P) - math.isqrt(256 * S) if squared else P - S


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside."""
    H, W = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    b[yd, xd] = a[ys, xs]
    return b


def basins_oracle(labels, h):
    """int64 [H, W]: the index of each foreground pixel's basin root, -1 on background."""
    H, W = labels.shape
    n = H * W
    idx = np.arange(n, dtype=np.int64).reshape(H, W)
    key = (h.astype(np.int64) << 31) | (np.int64((1 << 31) - 1) - idx)          # greater height, then smaller index
    best_key, best_idx = key.copy(), idx.copy()
    for dy, dx in NEIGHBOURS:
        same = (_shift(labels, dy, dx, 0) == labels)
        k = np.where(same, _shift(key, dy, dx, -1), -1)
        take = k > best_key
        best_key = np.where(take, k, best_key)
        best_idx = np.where(take, _shift(idx, dy, dx, -1), best_idx)
    ptr = best_idx.ravel().copy()
    while True:
        nxt = ptr[ptr]
        if np.array_equal(nxt, ptr):
            break
        ptr = nxt
    return np.where(labels.ravel() > 0, ptr, -1).reshape(H, W)


def saddles_oracle(labels, h, basin):
    """{(a, b): saddle} with a < b basin roots of one label that have 8-adjacent pixels."""
    out = {}
    hh = h.astype(np.int64)
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        lq, bq, hq = _shift(labels, dy, dx, 0), _shift(basin, dy, dx, -1), _shift(hh, dy, dx, 0)
        sel = (labels > 0) & (lq == labels) & (bq != basin)
        a, b = np.minimum(basin[sel], bq[sel]), np.maximum(basin[sel], bq[sel])
        s = np.minimum(hh[sel], hq[sel])
        for ai, bi, si in zip(a.tolist(), b.tolist(), s.tolist()):
            if out.get((ai, bi), -1) < si:
                out[(ai, bi)] = si
    return out


def _best_neighbours(edges, piece, hflat):
    """{u: (saddle, v)}: for every piece root u the neighbouring piece v with the greatest (saddle, key(root v))."""
    best = {}
    for (a, b), s in edges.items():
        u, v = piece[a], piece[b]
        if u == v:
            continue
        for x, y in ((u, v), (v, u)):
            cand = (s, int(hflat[y]), -y)
            if x not in best or cand > best[x]:
                best[x] = cand
    return {u: (c[0], -c[2]) for u, c in best.items()}


def split_oracle(labels, *, mask=None, conf=None, height=None, squared=None, min_depth=1.0, max_distance=None, max_rounds=64):
    """-> dict(labels int32 [H, W], regions, count, raw_basins, rounds, converged); regions also carries the integer
    accumulators first, sum_y, sum_x and, with conf, sum_conf."""
    labels = np.asarray(labels, dtype=np.int32)
    H, W = labels.shape
    if squared is None:
        squared = height is None
    h = heights_oracle(labels, max_distance) if height is None else np.asarray(height, dtype=np.int32)
    T = threshold(min_depth, squared)
    fg = labels > 0
    labels0 = np.where(fg, labels, 0)
    basin = basins_oracle(labels0, h)
    hflat = h.ravel().astype(np.int64)
    roots = np.unique(basin[fg]).tolist()
    edges = saddles_oracle(labels0, h, basin)
    piece = {r: r for r in roots}                                    # basin root -> root of its piece

    def key(r):
        return (int(hflat[r]), -r)

    rounds, converged = 0, False
    for _ in range(int(max_rounds)):
        best = _best_neighbours(edges, piece, hflat)
        nxt = {}
        for u, (s, v) in best.items():
            if depth(hflat[u], s, squared) <= T and key(v) > key(u):
                nxt[u] = v
        if not nxt:
            converged = True
            break
        rounds += 1
        for r in roots:
            p = piece[r]
            while p in nxt:
                p = nxt[p]
            piece[r] = p
    best = _best_neighbours(edges, piece, hflat)

    pflat = np.full(H * W, -1, dtype=np.int64)
    bf = basin.ravel()
    sel = np.flatnonzero(bf >= 0)
    lut = np.zeros(H * W, dtype=np.int64)
    for r in roots:
        lut[r] = piece[r]
    pflat[sel] = lut[bf[sel]]
    proots, first = np.unique(pflat[sel], return_index=True)         # first occurrence in row-major order
    first = sel[first]
    order = np.argsort(first, kind="stable")
    proots, first = proots[order], first[order]
    M = len(proots)
    ids = np.zeros(H * W, dtype=np.int32)
    ids[proots] = np.arange(1, M + 1, dtype=np.int32)
    out = np.zeros(H * W, dtype=np.int32)
    out[sel] = ids[pflat[sel]]

    yy, xx = np.divmod(np.arange(H * W, dtype=np.int64), W)
    area = np.zeros(M + 1, dtype=np.int64)
    sy, sx, sc = area.copy(), area.copy(), area.copy()
    lo = out.astype(np.int64)
    np.add.at(area, lo, 1)
    np.add.at(sy, lo, yy)
    np.add.at(sx, lo, xx)
    y0, x0 = np.full(M + 1, H, dtype=np.int32), np.full(M + 1, W, dtype=np.int32)
    y1, x1 = np.zeros(M + 1, dtype=np.int32), np.zeros(M + 1, dtype=np.int32)
    np.minimum.at(y0, lo, yy.astype(np.int32))
    np.minimum.at(x0, lo, xx.astype(np.int32))
    np.maximum.at(y1, lo, yy.astype(np.int32) + 1)
    np.maximum.at(x1, lo, xx.astype(np.int32) + 1)
    a = area[1:]
    cls = np.zeros(M, dtype=np.int32) if mask is None else np.asarray(mask, dtype=np.uint8).ravel()[first].astype(np.int32)
    reg = {"id": np.arange(1, M + 1, dtype=np.int32), "cls": cls, "area": a,
           "y0": y0[1:], "x0": x0[1:], "y1": y1[1:], "x1": x1[1:],
           "cy": sy[1:].astype(np.float64) / a, "cx": sx[1:].astype(np.float64) / a,
           "parent": labels.ravel()[first].astype(np.int32), "peak": hflat[proots].astype(np.int32),
           "peak_y": (proots // W).astype(np.int32), "peak_x": (proots % W).astype(np.int32),
           "saddle": np.array([best[int(r)][0] if int(r) in best else -1 for r in proots], dtype=np.int32).reshape(M),
           "first": first.astype(np.int64), "sum_y": sy[1:], "sum_x": sx[1:]}
    if conf is not None:
        c = np.clip(np.asarray(conf, dtype=np.float32), np.float32(0), np.float32(1)).astype(np.float64)
        np.add.at(sc, lo, np.rint(c * CONF_SCALE).astype(np.int64).ravel())
        reg["sum_conf"] = sc[1:]
        reg["mean_conf"] = sc[1:].astype(np.float64) / (a.astype(np.float64) * CONF_SCALE)
    return {"labels": out.reshape(H, W), "regions": reg, "count": M, "raw_basins": len(roots), "rounds": rounds,
            "converged": converged, "height": h}


# ---- the prototype shapes ------------------------------------------------------------------------------------------------
def disc(canvas, cy, cx, r, value=1):
    H, W = canvas.shape
    yy, xx = np.indices((H, W))
    canvas[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = value
    return canvas


def discs_map(H, W, centres=((0, 0), (0, 30)), r=20):
    """Discs of radius r under one label; `centres` are (dy, dx) offsets, the whole figure centred on the canvas."""
    m = np.zeros((H, W), dtype=np.int32)
    ys, xs = [c[0] for c in centres], [c[1] for c in centres]
    y = (H - (max(ys) + min(ys))) // 2
    x = (W - (max(xs) + min(xs))) // 2
    for dy, dx in centres:
        disc(m, y + dy, x + dx, r)
    return m


# three discs, centres 30 apart: one link along a row, one along the 18-24-30 triangle, whose oblique neck leaves a second
# summit in the middle disc (the fourth raw basin of the prototype)
CHAIN3 = ((0, 0), (0, 30), (18, 54))


def diagonal_bar_map(H, W, width=11, margin=6):
    """The pixels with |x - y - offset| <= width // 2, clipped `margin` from the canvas border."""
    m = np.zeros((H, W), dtype=np.int32)
    yy, xx = np.indices((H, W))
    inside = (yy >= margin) & (yy < H - margin) & (xx >= margin) & (xx < W - margin)
    m[(np.abs(xx - yy - (W - H) // 2) <= width // 2) & inside] = 1
    return m


def ellipse_map(H, W, a=40, b=12):
    """An ellipse of 80 x 24: half-axes a along x and b along y, centred."""
    m = np.zeros((H, W), dtype=np.int32)
    yy, xx = np.indices((H, W))
    cy, cx = H // 2, W // 2
    m[((xx - cx) * b) ** 2 + ((yy - cy) * a) ** 2 <= (a * b) ** 2] = 1
    return m


# (name, map builder(H, W), min_depth, raw basins, pieces, rounds): the outcomes of the rule's prototype
PROTOTYPE_CASES = (
    ("two_discs_shallow", lambda H, W: discs_map(H, W), 4.0, 2, 2, 0),
    ("two_discs_deep", lambda H, W: discs_map(H, W), 10.0, 2, 1, 1),
    ("three_discs_shallow", lambda H, W: discs_map(H, W, CHAIN3), 4.0, 4, 3, 1),
    ("three_discs_deep", lambda H, W: discs_map(H, W, CHAIN3), 10.0, 4, 1, 2),
    ("diagonal_bar", lambda H, W: diagonal_bar_map(H, W), 0.0, 3, 1, 1),
    ("ellipse", lambda H, W: ellipse_map(H, W), 0.0, 3, 1, 1),
)


# ---- maps of the tests ---------------------------------------------------------------------------------------------------
def random_labels(H, W, seed, n=7):
    """int32 [H, W]: a few rectangles and discs with distinct ids 1..n painted over one another (touching and nested) and a
    height map int32 in 0..7 to go with it: small ranges force plateaus, ties and many rounds."""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), dtype=np.int32)
    yy, xx = np.indices((H, W))
    for i in range(1, n + 1):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        a, b = int(rng.integers(6, H // 2)), int(rng.integers(6, W // 2))
        if rng.random() < 0.5:
            m[max(cy - a, 0):cy + a, max(cx - b, 0):cx + b] = i
        else:
            r = min(a, b)
            m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i
    return m, rng.integers(0, 8, size=(H, W)).astype(np.int32)


def speckle_labels(H, W, seed, fill=0.5):
    """int32 [H, W]: one label on a random `fill` of the pixels: many basins, many adjacent pairs."""
    return (np.random.default_rng(seed).random((H, W)) < fill).astype(np.int32)


def components_by_first_pixel(labels):
    """int32 [H, W]: the 8-connected components of equal positive labels, numbered 1.. by ascending smallest row-major pixel
    index (label_regions's numbering), by a plain flood fill."""
    labels = np.asarray(labels)
    H, W = labels.shape
    out = np.zeros((H, W), dtype=np.int32)
    n = 0
    for y0 in range(H):
        for x0 in range(W):
            if labels[y0, x0] <= 0 or out[y0, x0]:
                continue
            n += 1
            out[y0, x0] = n
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in NEIGHBOURS:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and not out[v, u] and labels[v, u] == labels[y0, x0]:
                        out[v, u] = n
                        stack.append((v, u))
    return out
