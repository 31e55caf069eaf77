"""The numpy restatement of insar_unet_ca_amd/focal.py (csrc/focal.hip): smoothing, rank filters and slope of a raster [H, W] or
[C, H, W] with the no-data rules of the scene tools. Vectorised with shifted slices of a zero-padded copy and int64, so that
GPU-sized cases stay fast; tests/test_focal_host.py pins it with an evaluator in Python integers that makes no use of
separability. Every function returns (out, out_valid) with out_valid uint8."""
import numpy as np

Q_LIMIT = (1 << 31) - 1
QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def validity(raster, valid=None, nodata=None):
    """bool, the raster's shape: inside is implied; the `valid` plane [H, W] is shared by the planes; `nodata` compares exactly
    in the raster's own type; a float32 pixel has to be finite."""
    r = np.asarray(raster)
    m = np.ones(r.shape, dtype=bool)
    if valid is not None:
        m &= (np.asarray(valid) != 0)                               # broadcasts over the planes
    if nodata is not None:
        m &= r != r.dtype.type(nodata)
    if r.dtype == np.float32:
        m &= np.isfinite(r)
    return m


def quantise(raster, scale):
    """int64 q: integer rasters as they are; float32 rint(clamp(float64(v) * scale, +-(2^31 - 1))), ties to even. Pixels that
    are not finite give 0 (they are invalid anyway)."""
    r = np.asarray(raster)
    if r.dtype != np.float32:
        return r.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.clip(np.nan_to_num(r.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) * np.float64(scale), -float(Q_LIMIT), float(Q_LIMIT))
    return np.rint(d).astype(np.int64)


def _planes(a):
    a = np.asarray(a)
    return a[None] if a.ndim == 2 else a


def _padded(a, R, fill=0):
    return np.pad(a, ((0, 0), (R, R), (R, R)), constant_values=fill)


def _invalid_value(dtype, fill):
    return QNAN if dtype == np.float32 else dtype.type(fill)


def threshold(min_coverage, S):
    return max(1, int(np.ceil(np.float64(min_coverage) * np.float64(S * S))))


def smooth(raster, taps, scale=2 ** 16, valid=None, nodata=None, min_coverage=0.0, keep_invalid=True, fill=0):
    r = np.asarray(raster)
    k = np.asarray(taps, dtype=np.int64)
    R, S = len(k) // 2, int(k.sum())
    m = _planes(validity(r, valid, nodata))
    q = _planes(quantise(r, scale)) * m
    P, H, W = q.shape
    qp, mp = _padded(q, R), _padded(m.astype(np.int64), R)
    A = np.zeros((P, H + 2 * R, W), dtype=np.int64)
    Wr = np.zeros_like(A)
    for i in range(2 * R + 1):                                      # rows: tap i multiplies the pixel at offset i - R
        A += k[i] * qp[:, :, i:i + W]
        Wr += k[i] * mp[:, :, i:i + W]
    N = np.zeros((P, H, W), dtype=np.int64)
    D = np.zeros_like(N)
    for j in range(2 * R + 1):
        N += k[j] * A[:, j:j + H]
        D += k[j] * Wr[:, j:j + H]
    ok = D >= threshold(min_coverage, S)
    if keep_invalid:
        ok &= m
    q_out = np.floor_divide(2 * N + D, np.where(ok, 2 * D, 1))       # floor: ties towards +infinity for both signs
    if r.dtype == np.float32:
        out = (q_out.astype(np.float64) / np.float64(scale)).astype(np.float32)
    else:
        out = q_out.astype(r.dtype)
    out = np.where(ok, out, _invalid_value(r.dtype, fill)).astype(r.dtype)
    return out.reshape(r.shape), ok.astype(np.uint8).reshape(r.shape)


def ordered_u32(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def from_ordered_u32(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def _keys(r):
    """int64 order keys, monotone in the value; for float32 a bijection of the bit pattern."""
    return ordered_u32(r).astype(np.int64).reshape(r.shape) if r.dtype == np.float32 else r.astype(np.int64)


def _from_keys(k, dtype):
    return from_ordered_u32(k.astype(np.uint32)).reshape(k.shape) if dtype == np.float32 else k.astype(dtype)


def rank(raster, op, radius, valid=None, nodata=None, min_count=1, keep_invalid=True, fill=0):
    r = np.asarray(raster)
    R = int(radius)
    m = _planes(validity(r, valid, nodata))
    key = _planes(_keys(r))
    P, H, W = key.shape
    BIG = np.int64(1) << np.int64(40)                               # above every key: invalid pixels sort last
    kp, mp = _padded(np.where(m, key, BIG), R, BIG), _padded(m.astype(np.int64), R)
    win = np.stack([kp[:, j:j + H, i:i + W] for j in range(2 * R + 1) for i in range(2 * R + 1)], axis=-1)
    n = sum(mp[:, j:j + H, i:i + W] for j in range(2 * R + 1) for i in range(2 * R + 1))
    if op == "min":
        chosen = win.min(axis=-1)
    elif op == "max":
        chosen = np.where(win == BIG, -BIG, win).max(axis=-1)
    else:
        srt = np.sort(win, axis=-1)
        at = np.maximum(n - 1, 0) // 2                              # the LOWER median of the n valid values
        chosen = np.take_along_axis(srt, at[..., None], axis=-1)[..., 0]
    ok = n >= int(min_count)
    if keep_invalid:
        ok &= m
    out = _from_keys(np.where(ok, chosen, 0), r.dtype)
    out = np.where(ok, out, _invalid_value(r.dtype, fill)).astype(r.dtype)
    return out.reshape(r.shape), ok.astype(np.uint8).reshape(r.shape)


def _slope(v, m, axis, h1, h2, keep_invalid):
    """One component along `axis` of [P, H, W]: float32 operations in a fixed order."""
    pad = [(0, 0)] * 3
    pad[axis] = (1, 1)
    vp, mp = np.pad(v, pad), np.pad(m, pad)
    n = v.shape[axis]
    sl = lambda a, o: np.take(a, np.arange(o, o + n), axis=axis)
    vm, v0, vq = sl(vp, 0), sl(vp, 1), sl(vp, 2)
    mm, m0, mq = sl(mp, 0), sl(mp, 1), sl(mp, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        central = ((vq - vm).astype(np.float32) * h2).astype(np.float32)
        forward = ((vq - v0).astype(np.float32) * h1).astype(np.float32)
        backward = ((v0 - vm).astype(np.float32) * h1).astype(np.float32)
    both, fwd, bwd = mm & mq, m0 & mq, m0 & mm
    ok = both | fwd | bwd
    if keep_invalid:
        ok &= m0
    g = np.where(both, central, np.where(fwd, forward, backward))
    return np.where(ok, g, QNAN).astype(np.float32), ok


def gradient(raster, spacing=(1.0, 1.0), valid=None, nodata=None, keep_invalid=True):
    r = np.asarray(raster, dtype=np.float32)
    m = _planes(validity(r, valid, nodata))
    v = np.where(m, _planes(r), np.float32(0))                       # invalid values are never used
    h = [np.float32(1.0 / float(d) / f) for d in spacing for f in (1.0, 2.0)]
    gy, oky = _slope(v, m, 1, h[0], h[1], keep_invalid)
    gx, okx = _slope(v, m, 2, h[2], h[3], keep_invalid)
    out = np.stack([gy, gx], axis=1)                                 # [P, 2, H, W]
    ok = (oky & okx).astype(np.uint8)
    return (out[0], ok[0]) if r.ndim == 2 else (out, ok)


# ---- data for the GPU tests ---------------------------------------------------------------------------------------------------
def speckle(shape, seed, holes=True):
    """float32 with a smooth part and noise; with `holes` NaN / +-inf pixels and, in a raster above 50 x 50, one NaN block of
    40 x 40, larger than any window."""
    rng = np.random.default_rng(seed)
    H, W = shape[-2:]
    yy, xx = np.mgrid[0:H, 0:W]
    a = (np.sin(yy / 7.0) * np.cos(xx / 5.0) + rng.standard_normal(shape) * 0.5).astype(np.float32)
    if holes:
        u = rng.random(shape)
        a[u < 0.06] = np.nan
        a[(u >= 0.06) & (u < 0.08)] = np.inf
        a[(u >= 0.08) & (u < 0.10)] = -np.inf
        if H > 50 and W > 50:
            a[..., H // 3:H // 3 + 40, W // 4:W // 4 + 40] = np.nan
    return a


def valid_plane(H, W, seed):
    rng = np.random.default_rng(seed)
    v = (rng.random((H, W)) > 0.15).astype(np.uint8)
    v[rng.random((H, W)) > 0.97] = 7                                 # any non-zero byte is valid
    return v
