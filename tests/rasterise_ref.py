"""A restatement of the polygon-rasterisation semantics (include/insar_hip.h, "polygon rasterisation") in numpy int64, one edge
at a time: the scanline form the kernels implement (`cover_vsum`, `rasterise`), and an independent evaluator for one pixel
centre by exact rational winding with fractions.Fraction (`winding_at`), which pins the scanline form in
tests/test_rasterise_host.py. Both take the int32 edge table [n, 5] = (X0, Y0, X1, Y1, value) in 1/256 pixel. The oracle of
tests/test_rasterise_gpu.py."""
from fractions import Fraction

import numpy as np

RANGES = {np.dtype(np.uint8): (0, 255), np.dtype(np.int32): (-(1 << 31), (1 << 31) - 1)}


def cover_vsum(edges, H, W):
    """int64 planes [H, W]: cover = sum of w, vsum = sum of w * value over the crossings of the pixel's row with c0 <= c."""
    dc = np.zeros((H, W + 1), dtype=np.int64)
    dv = np.zeros((H, W + 1), dtype=np.int64)
    for X0, Y0, X1, Y1, value in np.asarray(edges, dtype=np.int64).reshape(-1, 5).tolist():
        if Y0 == Y1:
            continue
        w = 1 if Y1 < Y0 else -1
        if Y0 > Y1:                                              # canonical order: both directions of a shared edge agree
            X0, Y0, X1, Y1 = X1, Y1, X0, Y0
        # Y0 <= 256 r + 128 < Y1  <=>  ceil((Y0 - 128) / 256) <= r < ceil((Y1 - 128) / 256)
        r0, r1 = max(-((128 - Y0) // 256), 0), min(-((128 - Y1) // 256), H)
        if r0 >= r1:
            continue
        rows = np.arange(r0, r1, dtype=np.int64)
        num = (X0 - 128) * (Y1 - Y0) + (X1 - X0) * (256 * rows + 128 - Y0)
        c0 = np.clip(-((-num) // (256 * (Y1 - Y0))), 0, W)      # one ceiling division; a crossing at c0 == W touches no pixel
        dc[rows, c0] += w                                        # one crossing per row: the indices are distinct
        dv[rows, c0] += w * value
    return np.cumsum(dc, axis=1)[:, :W], np.cumsum(dv, axis=1)[:, :W]


def decide(cover, vsum, dtype=np.uint8, fill=0, overlap_value=255, base=None):
    """(labels of `dtype`, number of pixels that became overlap_value because the polygons disagree)"""
    dtype = np.dtype(dtype)
    lo, hi = RANGES[dtype]
    bg = (cover == 0) & (vsum == 0)
    one = (cover == 1) & (vsum >= lo) & (vsum <= hi) & (vsum != overlap_value)
    out = np.full(cover.shape, fill, dtype=np.int64) if base is None else np.asarray(base).astype(np.int64)
    out = np.where(one, vsum, out)
    void = ~bg & ~one
    out = np.where(void, overlap_value, out)
    return out.astype(dtype), int(void.sum())


def rasterise(edges, H, W, dtype=np.uint8, fill=0, overlap_value=255, base=None):
    cover, vsum = cover_vsum(edges, H, W)
    return decide(cover, vsum, dtype, fill, overlap_value, base)


def winding_at(edges, r, c):
    """(cover, vsum) of pixel (r, c) by exact rational arithmetic, edge by edge: an edge counts iff it crosses the centre line
    of the row (half-open in Y) at an intercept Xi <= the centre's X (the top-left rule: on a left flank is inside)."""
    Yc, Xc = 256 * r + 128, 256 * c + 128
    cover = vsum = 0
    for X0, Y0, X1, Y1, value in np.asarray(edges, dtype=np.int64).reshape(-1, 5).tolist():
        if Y0 == Y1 or not min(Y0, Y1) <= Yc < max(Y0, Y1):
            continue
        xi = Fraction(X0) + Fraction(X1 - X0) * Fraction(Yc - Y0, Y1 - Y0)
        if xi <= Xc:
            w = 1 if Y1 < Y0 else -1
            cover += w
            vsum += w * value
    return cover, vsum


def crossings(edges, H):
    """The number of (edge, row of [0, H)) crossings, counted row by row."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 5)
    lo, hi = np.minimum(e[:, 1], e[:, 3]), np.maximum(e[:, 1], e[:, 3])
    yc = 256 * np.arange(H, dtype=np.int64) + 128
    return int(((lo[:, None] <= yc[None, :]) & (yc[None, :] < hi[:, None])).sum())
