"""The sequential restatement of contour lines (include/insar_hip.h, "contour lines"): a plain loop over levels, cells and
crossings that follows each line. It shares no code with insar_unet_ca_amd/contours.py or csrc/contour.hip: the segments come
from a table of the 16 cell masks (the device derives the successor of a crossing from a turn rule instead), the lines from
walking a dict. tests/test_contours_host.py pins it by its own invariants (exact fractions, point-in-polygon, contourpy)."""
import numpy as np

Q_LIMIT = (1 << 31) - 1
LINE_FIELDS = ("line", "level", "closed", "start", "count", "leader", "area2", "y0", "x0", "y1", "x1")

# cell corners: TL = 1, TR = 2, BR = 4, BL = 8 (set = above). Cell edges: T top, R right, B bottom, L left. A segment runs
# from the first edge to the second with the above side on its right ("Contour lines").
SEGMENTS = {0: (), 1: ("TL",), 2: ("RT",), 3: ("RL",), 4: ("BR",), 6: ("BT",), 7: ("BL",), 8: ("LB",), 9: ("TB",), 11: ("RB",),
            12: ("LR",), 13: ("TR",), 14: ("LT",), 15: ()}
SADDLES = {5: {True: ("TR", "BL"), False: ("TL", "BR")}, 10: {True: ("RB", "LT"), False: ("RT", "LB")}}     # joined / cut apart


def quantise(raster, scale=65536.0, valid=None, nodata=None):
    """(q int64 [H, W], ok bool [H, W]): zonal's rule, and which pixels are valid."""
    r = np.asarray(raster)
    if r.dtype == np.float32:
        ok = np.isfinite(r)
        d = np.where(ok, r, 0).astype(np.float64) * float(scale)
        q = np.rint(np.clip(d, -float(Q_LIMIT), float(Q_LIMIT))).astype(np.int64)
        if nodata is not None:
            ok &= r != np.float32(nodata)
    else:
        assert r.dtype in (np.uint8, np.int32)
        q = r.astype(np.int64)
        ok = np.ones(r.shape, dtype=bool)
        if nodata is not None:
            ok &= r != int(nodata)
    if valid is not None:
        ok &= np.asarray(valid) != 0
    return np.where(ok, q, 0), ok


def quantise_level(v, scale):
    return int(np.rint(min(max(float(v) * float(scale), -float(Q_LIMIT)), float(Q_LIMIT))))


def crossing_offset(q_p, q_n, q_l):
    """The offset 1..255 of the crossing from node p on the lattice edge p - n (exactly one of the two is above)."""
    above_p = q_p >= q_l
    qa, qb = (q_p, q_n) if above_p else (q_n, q_p)
    d = qa - qb
    s = min(max(((q_l - qb) * 512 + d) // (2 * d), 1), 255)
    return 256 - s if above_p else s


def cell_segments(tl, tr, br, bl, q_l):
    """The segments ("XY": from edge X to edge Y) of a cell of four valid nodes."""
    m = (tl >= q_l) | ((tr >= q_l) << 1) | ((br >= q_l) << 2) | ((bl >= q_l) << 3)
    if m in SADDLES:
        return SADDLES[m][tl + tr + br + bl >= 4 * q_l]
    return SEGMENTS[m]


def contours_oracle(raster, levels, scale=65536.0, valid=None, nodata=None):
    """What contour_lines returns, with numpy vertices, plus "succ" (dict crossing id -> crossing id) for the tests."""
    r = np.asarray(raster)
    H, W = r.shape
    q, ok = quantise(r, scale, valid, nodata)
    q = [[int(v) for v in row] for row in q]
    lscale = float(scale) if r.dtype == np.float32 else 1.0
    levels_q = [quantise_level(v, lscale) for v in levels]
    assert all(b > a for a, b in zip(levels_q, levels_q[1:]))
    N = H * W
    succ, pred, where = {}, {}, {}
    for l, q_l in enumerate(levels_q):
        for cy in range(H - 1):
            for cx in range(W - 1):
                if not (ok[cy, cx] and ok[cy, cx + 1] and ok[cy + 1, cx] and ok[cy + 1, cx + 1]):
                    continue
                p = cy * W + cx
                # crossing id and vertex of the four cell edges
                edge = {"T": ((l * N + p) * 2, cy, cx, 0), "B": ((l * N + p + W) * 2, cy + 1, cx, 0),
                        "L": ((l * N + p) * 2 + 1, cy, cx, 1), "R": ((l * N + p + 1) * 2 + 1, cy, cx + 1, 1)}
                for a, b in cell_segments(q[cy][cx], q[cy][cx + 1], q[cy + 1][cx + 1], q[cy + 1][cx], q_l):
                    ia, ib = edge[a][0], edge[b][0]
                    assert ia not in succ and ib not in pred
                    succ[ia], pred[ib] = ib, ia
                    for i, y, x, o in (edge[a], edge[b]):
                        off = crossing_offset(q[y][x], q[y + 1][x] if o else q[y][x + 1], q_l)
                        where[i] = (256 * y + 128 + (off if o else 0), 256 * x + 128 + (0 if o else off))
    ids = sorted(where)
    level_counts = np.zeros(len(levels_q), dtype=np.int64)
    for i in ids:
        level_counts[i // (2 * N)] += 1
    seen, lines = set(), []
    for i in ids:                                   # ascending: the first unseen crossing of a ring is its smallest
        if i in seen:
            continue
        start, closed = i, False
        while start in pred:
            start = pred[start]
            if start == i:
                closed = True
                break
        walk, k = [start], start
        seen.add(start)
        while k in succ and succ[k] != start:
            k = succ[k]
            assert k not in seen
            seen.add(k)
            walk.append(k)
        assert closed == (k in succ)
        lines.append((start, closed, walk))
    lines.sort(key=lambda t: t[0])
    vertices = np.zeros((len(ids), 2), dtype=np.int32)
    tab = {f: [] for f in LINE_FIELDS}
    at = 0
    for n, (leader, closed, walk) in enumerate(lines):
        v = [where[k] for k in walk]
        vertices[at:at + len(v)] = v
        area2 = sum(v[j][1] * v[(j + 1) % len(v)][0] - v[(j + 1) % len(v)][1] * v[j][0] for j in range(len(v))) if closed else 0
        row = dict(line=n, level=leader // (2 * N), closed=closed, start=at, count=len(v), leader=leader, area2=area2,
                   y0=min(y for y, _ in v), x0=min(x for _, x in v), y1=max(y for y, _ in v) + 1, x1=max(x for _, x in v) + 1)
        for f in LINE_FIELDS:
            tab[f].append(row[f])
        at += len(v)
    dt = {"area2": np.int64, "closed": np.bool_}
    return {"vertices": vertices, "lines": {f: np.asarray(tab[f], dtype=dt.get(f, np.int32)) for f in LINE_FIELDS},
            "n_lines": len(lines), "n_vertices": len(ids), "level_counts": level_counts,
            "levels_q": np.asarray(levels_q, dtype=np.int32), "scale": lscale, "succ": succ, "pred": pred}


# ---- host checkers the tests share ----------------------------------------------------------------------------------------------
def inside_even_odd(rings, py, px):
    """Even-odd over a list of int rings [(Y, X), ...]: the ray from (py, px) towards -x; exact integers."""
    n = 0
    for ring in rings:
        for j in range(len(ring)):
            (y0, x0), (y1, x1) = ring[j], ring[(j + 1) % len(ring)]
            if y0 > y1:
                y0, x0, y1, x1 = y1, x1, y0, x0
            if y0 <= py < y1 and (x1 - x0) * (py - y0) < (px - x0) * (y1 - y0):
                n += 1
    return bool(n & 1)


def smooth_map(H, W, seed, bumps=6, amp=100.0, smax=None):
    """float32: a sum of random Gaussian bumps and pits, in about +-amp, of widths up to smax (a fifth of the map)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W].astype(np.float64)
    f = np.zeros((H, W))
    for _ in range(bumps):
        cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.5, smax or 0.2 * max(H, W) + 2)
        f += rng.uniform(-amp, amp) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return f.astype(np.float32)


def bordered(m, low):
    """m with its border nodes set to `low`."""
    m = m.copy()
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = low
    return m
