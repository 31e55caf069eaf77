"""CPU restatement of insar_unet_ca_amd.hysteresis (a helper, not a test module): the candidate map, the components by a plain
flood fill, the seed rule, the numbering and the table, in numpy and plain Python, written from the rule of DESIGN.md's
"Hysteresis thresholds" and not from the kernels. Nothing here imports the package. tests/test_hysteresis_host.py pins it on
hand-built cases."""
from collections import deque

import numpy as np

CONF_SCALE = 1 << 30
TILE_H, TILE_W = 32, 64                  # the labelling tiles of csrc/regions.hip
SHAPES = [(1, 1), (1, 7), (5, 3), (33, 65), (64, 128), (97, 130)]
LOW, HIGH = 0.25, 0.75                   # the thresholds of the GPU comparison: multiples of 1/64, so equality occurs


def ordered_u32(x):
    """The order-preserving map of float32 bits to uint32: all bits of a negative flipped, the sign bit of the rest."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 == 1, ~u, u | np.uint32(1 << 31)).astype(np.uint32)


def per_class(v, K):
    """float32 [K] indexed by class from a number, a {class: number} dict (missing classes NaN) or a sequence of K numbers."""
    out = np.full(K, np.nan, dtype=np.float32)
    if isinstance(v, dict):
        for c, t in v.items():
            out[int(c)] = np.float32(t)
    elif np.ndim(v) == 0:
        out[:] = np.float32(v)
    else:
        out[:] = np.asarray(v, dtype=np.float32)
    return out


def candidates(score, low, high, classes=None, valid=None):
    """-> (cand uint8 [H, W], conf float32 [H, W], seed bool [H, W]). Plane 0 of a 3-D score never takes part; a 2-D score is
    the plane of class 1. Compares are float32; NaN compares false; the greatest score wins, ties go to the smallest class."""
    s = np.asarray(score, dtype=np.float32)
    planes = s[None] if s.ndim == 2 else s[1:]
    K = planes.shape[0] + 1
    lo, hi = per_class(low, K), per_class(high, K)
    sel = range(1, K) if classes is None else sorted(int(c) for c in classes)
    H, W = planes.shape[1:]
    cand = np.zeros((H, W), dtype=np.uint8)
    conf = np.zeros((H, W), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for c in sel:                                             # ascending: a later class must be strictly greater
            p = planes[c - 1]
            take = (p >= lo[c]) & ((cand == 0) | (p > conf))
            cand[take] = c
            conf[take] = p[take]
        if valid is not None:
            off = np.asarray(valid) == 0
            cand[off] = 0
            conf[off] = 0
        seed = (cand > 0) & (conf >= hi[cand])
    return cand, conf, seed


def flood(cand, connectivity=8):
    """-> int32 [H, W]: the components of equal non-zero class, numbered 1..M in the order a row-major scan meets them, which
    is ascending root (smallest row-major pixel index) order."""
    H, W = cand.shape
    comp = np.zeros((H, W), dtype=np.int32)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    m = 0
    for y0 in range(H):
        for x0 in range(W):
            if cand[y0, x0] == 0 or comp[y0, x0]:
                continue
            m += 1
            c = cand[y0, x0]
            comp[y0, x0] = m
            todo = deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                for dy, dx in steps:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and cand[v, u] == c and not comp[v, u]:
                        comp[v, u] = m
                        todo.append((v, u))
    return comp


def quantise_conf(conf):
    """int64 llrint(clamp(conf, 0, 1) * 2^30) of a float32 field (the product is exact; np.rint rounds half to even)."""
    c = np.clip(np.asarray(conf, dtype=np.float32), np.float32(0), np.float32(1)).astype(np.float64)
    return np.rint(c * CONF_SCALE).astype(np.int64)


def hysteresis(score, low, high, classes=None, valid=None, connectivity=8, min_area=1, min_seeds=1):
    """-> dict(labels, mask, conf, count, candidates, regions) as `hysteresis_regions` gives them, plus what the tests look at:
    cand, seed (the maps), root (per kept region) and unseeded (components of area >= min_area dropped by the seed rule alone)."""
    cand, conf, seed = candidates(score, low, high, classes, valid)
    H, W = cand.shape
    comp = flood(cand, connectivity)
    M = int(comp.max())
    flat = comp.ravel()
    area = np.bincount(flat, minlength=M + 1).astype(np.int64)
    n_seed = np.bincount(flat, weights=seed.ravel().astype(np.float64), minlength=M + 1).astype(np.int64)
    big = area >= min_area
    big[0] = False
    keep = big & (n_seed >= min_seeds)
    N = int(keep.sum())
    new_id = np.zeros(M + 1, dtype=np.int32)
    new_id[keep] = np.arange(1, N + 1, dtype=np.int32)
    labels = new_id[comp].astype(np.int32)
    mask = np.where(labels > 0, cand, 0).astype(np.uint8)
    q = quantise_conf(conf).ravel()
    cf = conf.ravel()
    f = {k: [] for k in ("cls", "area", "y0", "x0", "y1", "x1", "sum_y", "sum_x", "sum_conf", "root", "n_seed", "peak", "peak_y",
                         "peak_x")}
    for k in np.flatnonzero(keep):
        idx = np.flatnonzero(flat == k)                           # ascending: row-major order
        yy, xx = np.divmod(idx, W)
        first = idx[int(np.argmax(ordered_u32(cf[idx])))]         # argmax returns the first of equal keys
        for name, v in (("cls", cand.ravel()[idx[0]]), ("area", len(idx)), ("y0", yy.min()), ("x0", xx.min()), ("y1", yy.max() + 1),
                        ("x1", xx.max() + 1), ("sum_y", yy.sum()), ("sum_x", xx.sum()), ("sum_conf", q[idx].sum()), ("root", idx[0]),
                        ("n_seed", n_seed[k]), ("peak", cf[first]), ("peak_y", first // W), ("peak_x", first % W)):
            f[name].append(v)
    a = np.array(f["area"], dtype=np.int64).reshape(N)
    i32 = lambda name: np.array(f[name], dtype=np.int32).reshape(N)
    i64 = lambda name: np.array(f[name], dtype=np.int64).reshape(N)
    reg = {"id": np.arange(1, N + 1, dtype=np.int32), "cls": i32("cls"), "area": a, "y0": i32("y0"), "x0": i32("x0"), "y1": i32("y1"),
           "x1": i32("x1"), "cy": i64("sum_y").astype(np.float64) / a, "cx": i64("sum_x").astype(np.float64) / a,
           "mean_conf": i64("sum_conf").astype(np.float64) / (a.astype(np.float64) * CONF_SCALE), "n_seed": i64("n_seed"),
           "peak": np.array(f["peak"], dtype=np.float32).reshape(N), "peak_y": i32("peak_y"), "peak_x": i32("peak_x")}
    return {"labels": labels, "mask": mask, "conf": conf, "count": N, "candidates": int(big.sum()), "regions": reg,
            "cand": cand, "seed": seed, "root": i64("root"), "unseeded": int((big & ~keep).sum())}


def far_seeded(res):
    """The kept regions none of whose seeds lies in the 32 x 64 labelling tile of its root: their seeds reach the root only
    through the merge across tile borders."""
    H, W = res["labels"].shape
    out = []
    for k, root in zip(res["regions"]["id"], res["root"]):
        ys, xs = np.nonzero((res["labels"] == k) & res["seed"])
        tile = (root // W // TILE_H, root % W // TILE_W)
        if len(ys) and not ((ys // TILE_H == tile[0]) & (xs // TILE_W == tile[1])).any():
            out.append(int(k))
    return out


# ---- the maps ----------------------------------------------------------------------------------------------------------------
def blob_scores(H, W, seed, K=2):
    """float32 [K, H, W] (K = 1: [H, W], the one class plane): overlapping bumps of varied height over low-amplitude noise in
    every class plane, rounded to multiples of 1/64 so that pixels exactly equal to LOW and HIGH occur; plane 0 is one minus the
    greatest class score. Maps of at least 33 x 20 also carry, in class 1 and clear of the bumps, a faint patch without a
    confident pixel and a streak that starts in the first tile row and has its only confident pixel in the second; larger maps
    hold two NaN pixels."""
    rng = np.random.default_rng(seed)
    n_cls = max(1, K - 1)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    planes = rng.integers(-4, 9, size=(n_cls, H, W)).astype(np.float64) / 64.0
    for p in range(n_cls):
        for _ in range(max(1, H * W // 400)):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            sy, sx = rng.uniform(1.5, 7.0, size=2)
            height = rng.choice([0.4, 0.6, 0.75, 0.8, 1.0])
            planes[p] = np.maximum(planes[p], height * np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2)))
    planes = np.round(planes * 64.0) / 64.0
    if H >= 33 and W >= 20:
        planes[:, 0:9, 10:20] = 0.0                               # the faint patch: a component that only the seed rule drops
        planes[0, 2:7, 12:18] = 0.5
        planes[:, 18:H, 2:11] = 0.0                               # the streak: root at (20, 5), its one seed at (32, 6)
        planes[0, 20:33, 5:8] = 0.5
        planes[0, 32, 6] = 1.0
        planes[0, 15, 40] = np.nan
        planes[n_cls - 1, H - 1, W - 1] = np.nan
    planes = planes.astype(np.float32)
    if K == 1:
        return planes[0]
    with np.errstate(invalid="ignore"):
        bg = np.clip(1.0 - np.nan_to_num(planes, nan=0.0).max(axis=0), 0.0, 1.0).astype(np.float32)
    return np.concatenate([bg[None], planes], axis=0)


def valid_map(H, W, seed):
    """uint8 [H, W]: about one pixel in eight invalid (0), the rest 1 or 255."""
    rng = np.random.default_rng(seed + 12345)
    v = np.where(rng.random((H, W)) < 0.125, 0, 1).astype(np.uint8)
    v[rng.random((H, W)) < 0.1] *= 255
    return v
