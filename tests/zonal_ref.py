"""Numpy restatement of insar_unet_ca_amd/zonal.py on csrc/zonal.hip: per-region statistics of a raster over a label map,
everything in exact integers (Python ints for the square sums), ties of the extremes by an explicit first-index rule. Pinned
against a brute-force per-region loop in tests/test_zonal_host.py; the GPU tests compare with it exactly."""
import math

import numpy as np

Q_LIMIT = (1 << 31) - 1


def quantise(raster: np.ndarray, scale: float = 65536.0, nodata=None):
    """(q int64, valid bool, clipped bool) per pixel. Integer rasters: q = v. float32: the float64 product with `scale`,
    clamped to +-(2^31 - 1), rounded to nearest even."""
    if raster.dtype == np.float32:
        valid = np.isfinite(raster)
        if nodata is not None:
            valid &= ~(raster == np.float32(nodata))
        with np.errstate(all="ignore"):
            d = raster.astype(np.float64) * np.float64(scale)
        d = np.where(valid, d, 0.0)
        clipped = valid & ((d > Q_LIMIT) | (d < -Q_LIMIT))
        q = np.rint(np.clip(d, -float(Q_LIMIT), float(Q_LIMIT))).astype(np.int64)
    else:
        assert raster.dtype in (np.uint8, np.int32)
        q = raster.astype(np.int64)
        valid = np.ones(raster.shape, dtype=bool)
        if nodata is not None:
            valid &= q != int(nodata)
        clipped = np.zeros(raster.shape, dtype=bool)
    return q, valid, clipped


def quantise_scalar(v: float, scale: float) -> int:
    return int(np.rint(min(max(float(v) * float(scale), -float(Q_LIMIT)), float(Q_LIMIT))))


def _one_channel(labels, raster, N, max_regions, scale, nodata, bins, q_lo, q_hi):
    H, W = labels.shape
    lab = labels.ravel().astype(np.int64)
    q, valid, clipped = (a.ravel() for a in quantise(raster, scale, nodata))
    inside = (lab >= 1) & (lab <= max_regions)
    idx = np.arange(lab.size, dtype=np.int64)
    out = {k: np.zeros(N, dtype=np.int64) for k in ("n", "n_invalid", "n_clipped", "sum_q", "min_q", "max_q")}
    out["sumsq_q"] = np.zeros(N, dtype=object)
    out["argmin"] = np.full((N, 2), -1, dtype=np.int32)
    out["argmax"] = np.full((N, 2), -1, dtype=np.int32)
    if bins:
        out["hist"] = np.zeros((N, bins), dtype=np.int64)
        out["below"], out["above"] = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    # one stable sort by label: the pixels of a region in row-major order
    order = np.argsort(np.where(inside, lab, 0), kind="stable")
    ls = np.where(inside, lab, 0)[order]
    starts = np.searchsorted(ls, np.arange(1, N + 2), side="left")
    for r in range(N):
        px = order[starts[r]:starts[r + 1]]
        if px.size == 0:
            continue
        v = valid[px]
        out["n_invalid"][r] = int((~v).sum())
        px = px[v]
        out["n"][r] = px.size
        if px.size == 0:
            continue
        qr = q[px]
        out["n_clipped"][r] = int(clipped[px].sum())
        out["sum_q"][r] = int(qr.sum())
        out["sumsq_q"][r] = sum(int(x) * int(x) for x in qr.tolist())
        lo, hi = int(qr.min()), int(qr.max())
        out["min_q"][r], out["max_q"][r] = lo, hi
        first_lo, first_hi = int(px[qr == lo].min()), int(px[qr == hi].min())      # the first pixel that reaches it
        out["argmin"][r] = (first_lo // W, first_lo % W)
        out["argmax"][r] = (first_hi // W, first_hi % W)
        if bins:
            out["below"][r], out["above"][r] = int((qr < q_lo).sum()), int((qr >= q_hi).sum())
            for x in qr[(qr >= q_lo) & (qr < q_hi)].tolist():
                out["hist"][r, ((int(x) - q_lo) * bins) // (q_hi - q_lo)] += 1
    return out, int((lab > max_regions).sum())


def float_fields(out: dict, scale: float) -> None:
    """mean, std (population), min, max, sum in float64 from the integers: NaN where n == 0."""
    n = out["n"]
    shape = n.shape
    res = {k: np.full(n.size, np.nan) for k in ("mean", "std", "min", "max", "sum")}
    fn, fs, fss = n.ravel().tolist(), out["sum_q"].ravel().tolist(), out["sumsq_q"].ravel().tolist()
    fmin, fmax = out["min_q"].ravel().tolist(), out["max_q"].ravel().tolist()
    for i, k in enumerate(fn):
        if k == 0:
            continue
        res["mean"][i] = float(fs[i]) / (float(k) * scale)
        res["std"][i] = math.sqrt(k * fss[i] - fs[i] * fs[i]) / (float(k) * scale)
        res["min"][i], res["max"][i], res["sum"][i] = fmin[i] / scale, fmax[i] / scale, float(fs[i]) / scale
    for k, v in res.items():
        out[k] = v.reshape(shape)


def region_stats_ref(labels: np.ndarray, raster: np.ndarray, *, max_regions: int = 65536, count=None, scale: float = 65536.0,
                     nodata=None, bins: int = 0, range=None) -> dict:
    """What `insar_unet_ca_amd.region_stats` returns, from numpy arrays."""
    N = max_regions if count is None else count
    is_float = raster.dtype == np.float32
    s = float(scale) if is_float else 1.0
    q_lo = q_hi = 0
    if bins:
        q_lo, q_hi = quantise_scalar(range[0], s), quantise_scalar(range[1], s)
        assert q_lo < q_hi
    planes = raster[None] if raster.ndim == 2 else raster
    per = [_one_channel(labels, p, N, max_regions, scale, nodata, bins, q_lo, q_hi) for p in planes]
    out = {k: np.stack([p[0][k] for p in per]) for k in per[0][0]}
    float_fields(out, s)
    if raster.ndim == 2:
        out = {k: v[0] for k, v in out.items()}
    out["out_of_range"] = per[0][1]
    out["scale"], out["bins"], out["range_q"] = s, bins, (q_lo, q_hi)
    return out


INT_FIELDS = ("n", "n_invalid", "n_clipped", "sum_q", "sumsq_q", "min_q", "max_q", "argmin", "argmax")
HIST_FIELDS = ("hist", "below", "above")
FLOAT_FIELDS = ("mean", "std", "min", "max", "sum")
