"""Two independent numpy / Python restatements of insar_unet_ca_amd/reconstruct.py (csrc/reconstruct.hip): grey-scale
reconstruction of a raster [H, W] or [C, H, W] on order-preserving uint32 keys, with the no-data rules of the scene tools.

  (a) `flood`        a sequential priority flood: a heap by descending J; pop p, raise each neighbour q to min(J[p], G[q]) and push
                     it. Python integers on keys; a different algorithm from the kernel's.
  (b) `tile_jacobi`  the round structure of the kernels, parametrised by the tile edge T: each round solves every tile to its
                     LOCAL fixed point from the previous round's plane (a neighbour in another tile is read from that plane) and
                     the count of rounds up to the first that changes nothing is returned. The local solver is a plain Jacobi
                     iteration, not the kernel's sweeps: the local fixed point is unique. A tile that is not active (neither
                     it nor one of its 8 neighbours changed in the round before) cannot change, so solving it again is the
                     same as skipping it; the active tiles are counted as the kernels count them.

Both share `prepare` (keys, validity, the derived markers: outlets, raster -/+ h, key - 1) and `finish` (values, residue, extrema
map, fill), which restate the rules and nothing of the propagation. tests/test_reconstruct_host.py holds (a) == (b) and pins both
on cases with known answers."""
import heapq

import numpy as np

QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
PLAIN, FILL, HDOME, EXTREMA = 0, 1, 2, 3
ALL = np.uint32(0xFFFFFFFF)
SIGN = np.uint32(0x80000000)


def keys(x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.float32:
        u = x.view(np.uint32)
        return np.where(u & SIGN, ~u, u ^ SIGN).astype(np.uint32)
    if x.dtype == np.int32:
        return x.view(np.uint32) ^ SIGN
    assert x.dtype == np.uint8, x.dtype
    return x.astype(np.uint32)


def from_keys(k, dtype):
    k, dtype = np.ascontiguousarray(k, dtype=np.uint32), np.dtype(dtype)
    if dtype == np.float32:
        return np.where(k & SIGN, k ^ SIGN, ~k).astype(np.uint32).view(np.float32)
    if dtype == np.int32:
        return (k ^ SIGN).view(np.int32)
    assert dtype == np.uint8, dtype
    return k.astype(np.uint8)


def _planes(a):
    a = np.asarray(a)
    return a[None] if a.ndim == 2 else a


def _offsets(connectivity):
    assert connectivity in (4, 8)
    return [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and (connectivity == 8 or not (dy and dx))]


def validity(mask, marker=None, valid=None, nodata=None):
    """bool [P, H, W]: the `valid` plane [H, W] is shared by the planes; `nodata` compares exactly in the raster's own type, on
    mask and marker; a float32 mask pixel has to be finite, a float32 marker pixel must not be NaN (+-inf is a marker)."""
    g = _planes(mask)
    m = np.ones(g.shape, dtype=bool)
    if valid is not None:
        m &= (np.asarray(valid) != 0)
    if g.dtype == np.float32:
        m &= np.isfinite(g)
    if nodata is not None:
        m &= g != g.dtype.type(nodata)
    if marker is not None:
        f = _planes(marker)
        if f.dtype == np.float32:
            m &= ~np.isnan(f)
        if nodata is not None:
            m &= f != f.dtype.type(nodata)
    return m


def _shift_value(v, h, up):
    """raster + h (up) or raster - h: one float32 operation, or a saturating integer one."""
    if v.dtype == np.float32:
        with np.errstate(over="ignore", invalid="ignore"):
            return (v + np.float32(h)) if up else (v - np.float32(h))
    info = np.iinfo(v.dtype)
    return np.clip(v.astype(np.int64) + (int(h) if up else -int(h)), info.min, info.max).astype(v.dtype)


def prepare(mode, raster, marker=None, flip=False, connectivity=8, h=None, valid=None, nodata=None):
    """(J0, G, ok): the start plane min(F, G) and the mask keys, uint32 [P, H, W], invalid pixels 0; ok bool [P, H, W]."""
    g = _planes(raster)
    ok = validity(g, marker if mode == PLAIN else None, valid, nodata)
    x = ALL if flip else np.uint32(0)
    G = np.where(ok, keys(g) ^ x, np.uint32(0)).astype(np.uint32)
    if mode == PLAIN:
        F = keys(_planes(marker)) ^ x
    elif mode == FILL:
        pad = np.pad(ok, ((0, 0), (1, 1), (1, 1)), constant_values=False)
        P, H, W = ok.shape
        outlet = np.zeros_like(ok)
        for dy, dx in _offsets(connectivity):
            outlet |= ~pad[:, 1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
        F = np.where(outlet, G, np.uint32(0))
    elif mode == HDOME:
        F = keys(_shift_value(g, h, bool(flip))) ^ x
    else:
        F = np.where(G > 0, G - np.uint32(1), np.uint32(0))
    J = np.where(ok, np.minimum(F.astype(np.uint32), G), np.uint32(0)).astype(np.uint32)
    return J, G, ok


# ---- (a) the priority flood ------------------------------------------------------------------------------------------------------
def flood(J0, G, connectivity=8):
    """The fixed point of J <- min(G, max over the neighbourhood) from J0 <= G, uint32 [P, H, W], by a widest-path flood."""
    out = np.empty_like(J0)
    offs = _offsets(connectivity)
    for p in range(J0.shape[0]):
        H, W = J0.shape[1:]
        J = [int(v) for v in J0[p].ravel()]
        g = [int(v) for v in G[p].ravel()]
        heap = [(-v, i) for i, v in enumerate(J) if v > 0]
        heapq.heapify(heap)
        while heap:
            nv, i = heapq.heappop(heap)
            v = -nv
            if v != J[i]:
                continue                                             # raised since it was pushed: a later entry stands for it
            y, x = divmod(i, W)
            for dy, dx in offs:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W:
                    q = yy * W + xx
                    c = v if v < g[q] else g[q]
                    if c > J[q]:
                        J[q] = c
                        heapq.heappush(heap, (-c, q))
        out[p] = np.array(J, dtype=np.uint32).reshape(H, W)
    return out


# ---- (b) the tile-Jacobi rounds -----------------------------------------------------------------------------------------------------
def _tile_any(changed, T):
    """bool [tiles_y, tiles_x]: whether any pixel of a tile is set."""
    H, W = changed.shape
    ty, tx = -(-H // T), -(-W // T)
    pad = np.zeros((ty * T, tx * T), dtype=bool)
    pad[:H, :W] = changed
    return pad.reshape(ty, T, tx, T).any(axis=(1, 3))


def _grow(tiles):
    """A tile or one of its 8 neighbours is set."""
    p = np.pad(tiles, 1, constant_values=False)
    out = np.zeros_like(tiles)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= p[dy:dy + tiles.shape[0], dx:dx + tiles.shape[1]]
    return out


def tile_jacobi(J0, G, connectivity=8, T=64, max_rounds=None):
    """(R, rounds, converged, active_tile_rounds) of uint32 [P, H, W] planes. `rounds` counts up to and including the first round
    in which no tile of any plane changed; with `max_rounds` the planes stop there and `converged` says whether that round was
    reached. The planes run in the same rounds, as one launch serves them all."""
    P, H, W = J0.shape
    offs = _offsets(connectivity)
    yy, xx = np.mgrid[0:H, 0:W]
    same = {(dy, dx): ((yy + dy) // T == yy // T) & ((xx + dx) // T == xx // T) for dy, dx in offs}
    out = np.empty_like(J0)
    rounds, converged, active_total = 0, True, 0
    for p in range(P):
        J, g = J0[p].copy(), G[p]
        active = np.ones((-(-H // T), -(-W // T)), dtype=bool)
        r, done = 0, False
        while not done and (max_rounds is None or r < max_rounds):
            prev = np.pad(J, 1, constant_values=0)
            cur = J
            while True:
                cp = np.pad(cur, 1, constant_values=0)
                m = cur
                for dy, dx in offs:
                    sl = (slice(1 + dy, H + 1 + dy), slice(1 + dx, W + 1 + dx))
                    m = np.maximum(m, np.where(same[(dy, dx)], cp[sl], prev[sl]))
                new = np.minimum(g, m)
                if np.array_equal(new, cur):
                    break
                cur = new
            changed = _tile_any(cur != J, T)
            assert not (changed & ~active).any()                     # an inactive tile cannot change
            active_total += int(active.sum())
            J, r = cur, r + 1
            done = not changed.any()
            active = _grow(changed)
        out[p] = J
        rounds, converged = max(rounds, r), converged and done
    return out, rounds, converged, active_total


# ---- finish ---------------------------------------------------------------------------------------------------------------------------
def finish(R, G, raster, ok, flip=False, fill=0):
    """out (the raster's dtype), residue (float32 / int32, never negative), extrema (uint8) and valid (uint8), each in the raster's
    shape: keys back to values; NaN / `fill` and NaN / 0 at invalid pixels."""
    g = _planes(raster)
    x = ALL if flip else np.uint32(0)
    rec = from_keys(R ^ x, g.dtype)
    if g.dtype == np.float32:
        with np.errstate(invalid="ignore", over="ignore"):
            res = (rec - g) if flip else (g - rec)
        out, res = np.where(ok, rec, QNAN).astype(np.float32), np.where(ok, res, QNAN).astype(np.float32)
    else:
        a, b = rec.astype(np.int64), g.astype(np.int64)
        res = np.minimum((a - b) if flip else (b - a), (1 << 31) - 1)
        out, res = np.where(ok, rec, g.dtype.type(fill)).astype(g.dtype), np.where(ok, res, 0).astype(np.int32)
    shape = np.asarray(raster).shape
    return {"out": out.reshape(shape), "residue": res.reshape(shape), "extrema": (ok & (G > R)).astype(np.uint8).reshape(shape),
            "valid": ok.astype(np.uint8).reshape(shape)}


def _solve(J, G, connectivity, solver, max_rounds):
    if solver == "flood":
        assert max_rounds is None
        return flood(J, G, connectivity), None, True, None
    kind, T = solver
    assert kind == "jacobi"
    return tile_jacobi(J, G, connectivity, T, max_rounds)


def run(mode, raster, marker=None, flip=False, connectivity=8, h=None, valid=None, nodata=None, fill=0, solver="flood", max_rounds=None):
    """Every output of one call, with "rounds", "converged" and "active_tile_rounds" (None from the flood)."""
    J, G, ok = prepare(mode, raster, marker, flip, connectivity, h, valid, nodata)
    R, rounds, converged, active = _solve(J, G, connectivity, solver, max_rounds)
    res = finish(R, G, raster, ok, flip, fill)
    res.update(rounds=rounds, converged=converged, active_tile_rounds=active)
    return res


def reconstruct(marker, mask, method="dilation", **kw):
    return run(PLAIN, mask, marker, flip=method == "erosion", **kw)


def fill_sinks(raster, invert=False, **kw):
    return run(FILL, raster, flip=not invert, **kw)


def h_dome(raster, h, invert=False, **kw):
    return run(HDOME, raster, h=h, flip=invert, **kw)


def regional_extrema(raster, kind="max", **kw):
    return run(EXTREMA, raster, flip=kind == "min", **kw)


# ---- inputs the host and GPU tests share ------------------------------------------------------------------------------------------------
def random_raster(shape, dtype, seed):
    """A raster with heavy ties and the awkward values of its type: float32 +-0.0, +-inf, NaN and -9999 (a nodata value);
    int32 INT32_MIN and INT32_MAX; uint8 eight levels."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return rng.integers(0, 8, size=shape).astype(np.uint8) * np.uint8(31)
    if dtype == np.int32:
        a = rng.integers(-5, 6, size=shape).astype(np.int64) * 500_000_000
        return np.clip(a, -(1 << 31), (1 << 31) - 1).astype(np.int32)          # +-5 (2.5e9) saturate to INT32_MIN and INT32_MAX
    a = np.round(rng.normal(size=shape) * 4).astype(np.float32) / np.float32(4)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -9999.0], dtype=np.float32)
    pick = rng.random(size=shape) < 0.08
    return np.where(pick, special[rng.integers(0, len(special), size=shape)], a).astype(np.float32)


def cut_plane(H, W, seed):
    """uint8 [H, W]: a valid plane whose zero lines cut the raster into components, with a few zero pixels besides."""
    rng = np.random.default_rng(seed)
    v = (rng.random(size=(H, W)) > 0.03).astype(np.uint8)
    v[H // 2, :] = 0
    v[:, W // 3] = 0
    if H > 2 and W > 2:
        v[H // 2, W // 2 + 1] = 1                                    # a one-pixel gate in the horizontal cut
    return v


def serpentine(H, W):
    """(marker, mask) uint8 [H, W]: a one-pixel-wide corridor of value 200 that runs along every second row and turns at alternate
    ends, in a mask of 10; the marker is 200 at the corridor's first pixel and 0 elsewhere. At connectivity 4 and 8 alike the
    only way through is along the corridor."""
    mask = np.full((H, W), 10, dtype=np.uint8)
    for i, y in enumerate(range(0, H, 2)):
        mask[y, :] = 200
        if y + 2 < H:
            mask[y + 1, W - 1 if i % 2 == 0 else 0] = 200
    marker = np.zeros((H, W), dtype=np.uint8)
    marker[0, 0] = 200
    return marker, mask
