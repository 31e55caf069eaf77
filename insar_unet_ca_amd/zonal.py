"""Statistics of a raster over the regions of a label map on the device (csrc/zonal.hip: insar_zonal_clear / _accumulate):
what `scipy.ndimage` does after `labels.cpu()`, without the copy. `labels` is what `label_regions`, `rasterise_polygons(int32)`
or any other stage left on the device; the raster is the scene itself or a co-registered map (coherence, displacement, a DEM,
the d2 map of `distance_transform`).

Semantics: labels 1..max_regions are measured, 0 and negative labels are background, pixels with a larger label are counted
in `out_of_range` and nothing else. Per pixel the raster value becomes an integer q: integer rasters q = v; float32
q = rint(clamp(float64(v) * scale, -(2^31 - 1), 2^31 - 1)), ties to even. A clamped pixel is counted in `n_clipped` and takes
part with the clamped q; a pixel that is not finite, or equals `nodata` in the raster's own type, is counted in `n_invalid`
and takes no other part. Everything the device accumulates is an integer (the square sum exactly, in two 64-bit words), so
the table is bitwise reproducible; the float fields are formed on the host in float64 from those integers.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_on_device, query_bytes, read_back
from .regions import DEFAULT_MAX_REGIONS

MAX_CHANNELS = 4
MAX_BINS = 256
Q_LIMIT = (1 << 31) - 1

# the C struct InsarZonalStat (include/insar_hip.h); record 0 of a table is the header, whose `sum_q` is out_of_range
ZONAL_DTYPE = np.dtype([("sum_q", "<i8"), ("sumsq_lo", "<u8"), ("sumsq_hi", "<u8"), ("min_key", "<u8"), ("max_key", "<u8"),
                        ("n", "<i4"), ("n_invalid", "<i4"), ("n_clipped", "<i4"), ("below", "<u4"), ("above", "<u4"),
                        ("_pad", "<i4")])
assert ZONAL_DTYPE.itemsize == 64

_ELEM = {torch.float32: _lib.ZONAL_F32, torch.uint8: _lib.ZONAL_U8, torch.int32: _lib.ZONAL_I32}


def scratch_bytes(max_regions: int = DEFAULT_MAX_REGIONS, bins: int = 0, channels: int = 1) -> int:
    """Bytes of the table for max_regions regions, `bins` histogram bins and `channels` channels. Host arithmetic only."""
    return query_bytes("insar_zonal_scratch_bytes", max_regions, bins, channels, outputs=1)


class ZonalScratch(Scratch):
    """The device table of one (max_regions, bins, channels) and the pinned host copy it is read back into. Nothing in it
    has to survive between calls. `table`: a contiguous uint8 device tensor of exactly `scratch_bytes(...)` bytes, 16-byte
    aligned, to use instead of a fresh allocation (a view into a larger buffer, for instance)."""
    KEY = ("max_regions", "bins", "channels")

    def __init__(self, device: torch.device, max_regions: int = DEFAULT_MAX_REGIONS, bins: int = 0, channels: int = 1,
                 table: Optional[torch.Tensor] = None):
        tb = scratch_bytes(max_regions, bins, channels)
        super().__init__((max_regions, bins, channels), device, table=self.adopt_table("ZonalScratch", table, tb), host=tb)


def quantise_scalar(v: float, scale: float) -> int:
    """q of one float64 value: the device rule, for the histogram edges."""
    d = min(max(float(v) * float(scale), -float(Q_LIMIT)), float(Q_LIMIT))
    return int(np.rint(d))


def _check_args(labels, raster, max_regions, count, scale, nodata, bins, range_, scratch=None):
    """Every refusal, none of which needs a device; the one of host tensors comes last, so that the others can be met on the
    host. Returns (channels, has_nodata, nodata, q_lo, q_hi)."""
    who = "region_stats"
    if not isinstance(labels, torch.Tensor) or not isinstance(raster, torch.Tensor):
        raise InsarError(f"region_stats: labels and raster must be torch tensors, got {type(labels).__name__}, {type(raster).__name__}")
    if labels.dtype != torch.int32 or labels.dim() != 2:
        raise InsarError(f"region_stats: labels must be a 2-D int32 tensor, got {labels.dtype} {tuple(labels.shape)}")
    H, W = labels.shape
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise InsarError(f"region_stats: map {H} x {W}: need H, W >= 1 and H * W < 2^31")
    if raster.dtype not in _ELEM:
        raise InsarError(f"region_stats: raster dtype {raster.dtype}: float32, uint8 or int32")
    if raster.dim() not in (2, 3) or tuple(raster.shape[-2:]) != (H, W):
        raise InsarError(f"region_stats: raster must be [{H}, {W}] or [C, {H}, {W}], got {tuple(raster.shape)}")
    channels = 1 if raster.dim() == 2 else int(raster.shape[0])
    if not 1 <= channels <= MAX_CHANNELS:
        raise InsarError(f"region_stats: {channels} channels: 1..{MAX_CHANNELS}")
    if not labels.is_contiguous() or not raster.is_contiguous():
        raise InsarError("region_stats: labels and raster must be contiguous")
    check_int(who, "max_regions", max_regions, 1, 1 << 24, integral_floats=True)
    if count is not None:
        check_int(who, "count", count, 0, max_regions, integral_floats=True, expect=f"an integer in 0..max_regions={max_regions}")
    try:
        scale_ok = math.isfinite(float(scale)) and float(scale) > 0
    except (TypeError, ValueError):
        scale_ok = False
    if not scale_ok:
        raise InsarError(f"scale={scale!r}: a positive finite number")
    has_nodata, nd = 0, 0.0
    if nodata is not None:
        nd = float(nodata)
        if math.isnan(nd):
            raise InsarError("nodata is NaN: NaN pixels are invalid already, and nothing equals NaN")
        if raster.dtype != torch.float32:
            lo_t, hi_t = (0, 255) if raster.dtype == torch.uint8 else (-(1 << 31), (1 << 31) - 1)
            if nd != int(nd) or not lo_t <= int(nd) <= hi_t:
                raise InsarError(f"nodata={nodata!r} is no value of a {raster.dtype} raster")
        has_nodata = 1
    check_int(who, "bins", bins, 0, MAX_BINS, integral_floats=True)
    q_lo = q_hi = 0
    if bins > 0:
        try:
            lo, hi = (float(range_[0]), float(range_[1])) if range_ is not None and len(range_) == 2 else (math.nan, math.nan)
        except (TypeError, ValueError):
            lo = hi = math.nan
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise InsarError(f"range={range_!r}: bins > 0 needs a finite (lo, hi)")
        qs = float(scale) if raster.dtype == torch.float32 else 1.0
        q_lo, q_hi = quantise_scalar(lo, qs), quantise_scalar(hi, qs)
        if q_lo >= q_hi:
            raise InsarError(f"range={range_!r}: lo >= hi after quantisation ({q_lo} >= {q_hi})")
    key = (int(max_regions), int(bins), channels)
    if scratch is not None:
        ZonalScratch.check(who, scratch, key, table_bytes=scratch_bytes(*key))
    check_on_device(who, "labels", labels)
    check_on_device(who, "raster", raster, like=labels)
    if scratch is not None and scratch.table.device != labels.device:
        raise InsarError(f"{who}: the scratch lives on {scratch.table.device}, labels on {labels.device}")
    return channels, has_nodata, nd, q_lo, q_hi


def _exact_moments(n: np.ndarray, sum_q: np.ndarray, lo: np.ndarray, hi: np.ndarray):
    """(the square sums lo + (hi << 32) as Python ints, sqrt(n * sumsq - sum^2) in float64) over the records with n > 0; the
    numerator is formed in exact integers before the one square root. Records whose numerator's terms stay below 2^62 take
    int64 arithmetic (exact there, and the conversion to float64 rounds as Python's does), the others Python ints."""
    sumsq = np.zeros(n.shape, dtype=object)
    root = np.zeros(n.shape, dtype=np.float64)
    fs, fr = sumsq.reshape(-1), root.reshape(-1)
    fn, fq, fl, fh = n.reshape(-1), sum_q.reshape(-1), lo.reshape(-1), hi.reshape(-1)
    has = fn > 0
    nf, qf = fn.astype(np.float64), fq.astype(np.float64)
    ss_est = fl.astype(np.float64) + fh.astype(np.float64) * 4294967296.0
    small = has & (fh < np.uint64(1 << 30)) & (fl < np.uint64(1 << 62)) & (nf * ss_est < 2.0 ** 62) & (np.abs(qf) < 2.0 ** 31)
    i = np.flatnonzero(small)
    ss = fl[i] + (fh[i] << np.uint64(32))                          # < 2^63: uint64 holds it
    fs[i] = ss.astype(object)
    fr[i] = np.sqrt((fn[i] * ss.astype(np.int64) - fq[i] * fq[i]).astype(np.float64))
    for k in np.flatnonzero(has & ~small).tolist():
        big = int(fl[k]) + (int(fh[k]) << 32)
        fs[k] = big
        fr[k] = math.sqrt(int(fn[k]) * big - int(fq[k]) ** 2)
    return sumsq, root


def stats_from_table(raw: np.ndarray, *, max_regions: int, channels: int, bins: int, count: Optional[int], shape, scale: float,
                     is_float: bool, q_range=(0, 0), squeeze: bool = True) -> Dict[str, object]:
    """The result of `region_stats` (fresh arrays) from the raw bytes of a device table. `shape` = (H, W) of the map; `scale`
    divides the float fields (1 for an integer raster)."""
    H, W = int(shape[0]), int(shape[1])
    N = int(max_regions if count is None else count)
    nrec = 1 + channels * max_regions
    rec = raw[:64 * nrec].view(ZONAL_DTYPE)
    r = rec[1:].reshape(channels, max_regions)[:, :N]
    n = r["n"].astype(np.int64)
    has = n > 0
    sum_q = r["sum_q"].astype(np.int64)
    sumsq, num = _exact_moments(n, sum_q, r["sumsq_lo"], r["sumsq_hi"])
    bias = np.int64(1) << np.int64(31)
    min_q = np.where(has, (r["min_key"] >> np.uint64(32)).astype(np.int64) - bias, 0)
    max_q = np.where(has, (r["max_key"] >> np.uint64(32)).astype(np.int64) - bias, 0)
    imin = (r["min_key"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    imax = (~r["max_key"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    argmin = np.where(has[..., None], np.stack([imin // W, imin % W], axis=-1), -1).astype(np.int32)
    argmax = np.where(has[..., None], np.stack([imax // W, imax % W], axis=-1), -1).astype(np.int32)
    s = float(scale) if is_float else 1.0
    nf = np.where(has, n, 1).astype(np.float64)
    nan = np.float64("nan")
    out: Dict[str, object] = {
        "n": n, "n_invalid": r["n_invalid"].astype(np.int64), "n_clipped": r["n_clipped"].astype(np.int64), "sum_q": sum_q,
        "sumsq_q": sumsq, "min_q": min_q, "max_q": max_q, "argmin": argmin, "argmax": argmax,
        "mean": np.where(has, sum_q.astype(np.float64) / (nf * s), nan), "std": np.where(has, num / (nf * s), nan),
        "min": np.where(has, min_q.astype(np.float64) / s, nan), "max": np.where(has, max_q.astype(np.float64) / s, nan),
        "sum": np.where(has, sum_q.astype(np.float64) / s, nan)}
    if bins > 0:
        hist = raw[64 * nrec:64 * nrec + 4 * channels * max_regions * bins].view("<u4").reshape(channels, max_regions, bins)
        out["hist"] = hist[:, :N].astype(np.int64)
        out["below"], out["above"] = r["below"].astype(np.int64), r["above"].astype(np.int64)
    if squeeze:
        out = {k: v[0] for k, v in out.items()}
    out["out_of_range"] = int(rec["sum_q"][0])
    out["scale"], out["bins"], out["range_q"] = s, int(bins), (int(q_range[0]), int(q_range[1]))
    return out


def percentile(stats: Dict[str, object], p: float) -> np.ndarray:
    """The p-th percentile (0..100) of the valid pixels of every region from the histogram of `region_stats(..., bins > 0)`,
    in raster units. With t = p / 100 * n the value lies in the first non-empty bin b whose cumulative count (the pixels
    `below` included) reaches t, at edge_b + (t - count before b) / hist[b] * bin width; t inside `below` gives the lower end
    of the range, t beyond the last bin its upper end; NaN where n == 0."""
    if "hist" not in stats:
        raise InsarError("percentile: the statistics hold no histogram (region_stats(..., bins > 0, range=(lo, hi)))")
    if not 0 <= p <= 100:
        raise InsarError(f"percentile: p={p!r} outside 0..100")
    hist = np.asarray(stats["hist"], dtype=np.float64)
    below, n = np.asarray(stats["below"], dtype=np.float64), np.asarray(stats["n"], dtype=np.float64)
    bins = hist.shape[-1]
    q_lo, q_hi = stats["range_q"]
    width = (q_hi - q_lo) / bins
    t = (p / 100.0) * n
    cum = below[..., None] + np.cumsum(hist, axis=-1)
    before = cum - hist
    ok = (cum >= t[..., None]) & (hist > 0)
    b = np.argmax(ok, axis=-1)
    pick = lambda a: np.take_along_axis(a, b[..., None], axis=-1)[..., 0]
    frac = np.clip((t - pick(before)) / np.where(pick(hist) > 0, pick(hist), 1.0), 0.0, 1.0)
    q = np.where(ok.any(axis=-1), q_lo + (b + frac) * width, float(q_hi))
    return np.where(n > 0, q / stats["scale"], np.nan)


def region_stats(labels: torch.Tensor, raster: torch.Tensor, *, max_regions: int = DEFAULT_MAX_REGIONS, count: Optional[int] = None,
                 scale: float = 65536.0, nodata: Optional[float] = None, bins: int = 0, range=None,
                 scratch: Optional[ZonalScratch] = None) -> dict:
    """Per-region statistics of a device raster over a device label map.

        st = region_stats(det["labels"], coherence, count=det["count"])        # rows aligned with det["regions"]["id"]
        st["n"], st["n_invalid"], st["n_clipped"], st["sum_q"], st["min_q"], st["max_q"]   int64 [N]
        st["sumsq_q"]  object [N] of Python ints (exact)       st["argmin"], st["argmax"]  int32 [N, 2] as (y, x), -1 where n == 0
        st["mean"], st["std"] (population), st["min"], st["max"], st["sum"]               float64 [N], NaN where n == 0
        st["hist"] int64 [N, bins], st["below"], st["above"]   with bins > 0 and range=(lo, hi) in raster units
        st["out_of_range"]  pixels whose label exceeds max_regions

    N is `count` if given, else max_regions; a [C, H, W] raster gives [C, N] arrays. Integer rasters ignore `scale` (q = v,
    the float fields are q itself). Two launches on the current stream and ONE device-to-host read-back. `scratch`: a
    ZonalScratch of this (max_regions, bins, channels) to reuse (else allocated)."""
    channels, has_nodata, nd, q_lo, q_hi = _check_args(labels, raster, max_regions, count, scale, nodata, bins, range, scratch)
    H, W = labels.shape
    max_regions, bins = int(max_regions), int(bins)
    if scratch is None:
        scratch = ZonalScratch(labels.device, max_regions, bins, channels)
    with torch.cuda.device(labels.device):
        s = _lib.stream_ptr()
        call("insar_zonal_clear", ptr(scratch.table), max_regions, bins, channels, s)
        call("insar_zonal_accumulate", ptr(labels), ptr(raster), _ELEM[raster.dtype], channels, H, W, float(scale), has_nodata, nd,
             bins, q_lo, q_hi, max_regions, ptr(scratch.table), s)
        raw = read_back(scratch.host, scratch.table)
    return stats_from_table(raw, max_regions=max_regions, channels=channels, bins=bins, count=count, shape=(H, W),
                            scale=float(scale), is_float=raster.dtype == torch.float32, q_range=(q_lo, q_hi),
                            squeeze=raster.dim() == 2)
