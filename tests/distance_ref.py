"""Numpy oracles of insar_unet_ca_amd/distance.py, written from the definitions (include/insar_hip.h, "distance transform"),
not from the kernels. Pinned by tests/test_distance_host.py against an all-pairs brute force and scipy's exact EDT.

Every function takes ONE image [H, W]; the tests loop over a batch."""
import numpy as np

FAR = 0x7FFFFFFF


def sites_oracle(m, sites="edge", ignore_value=None):
    """bool [H, W]: ("eq", v) m == v; ("ne", v) m != v; "edge": m[p] is not ignored and a 4-neighbour q inside the image is
    neither ignored nor equal to m[p]."""
    m = np.asarray(m).astype(np.int64)
    if sites != "edge":
        kind, v = sites
        return (m == v) if kind == "eq" else (m != v)
    live = np.ones(m.shape, dtype=bool) if ignore_value is None else m != ignore_value
    out = np.zeros(m.shape, dtype=bool)
    for axis in (0, 1):
        a, b = [slice(None)] * 2, [slice(None)] * 2
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        differ = live[a] & live[b] & (m[a] != m[b])
        out[a] |= differ
        out[b] |= differ
    return out


def cap(d2, max_distance):
    """int32: values above max_distance^2 (and the INF of `dist_oracle`) become FAR."""
    d2 = np.asarray(d2, dtype=np.int64)
    limit = FAR - 1 if max_distance is None else int(max_distance) ** 2
    return np.where(d2 <= limit, d2, FAR).astype(np.int32)


def dist_oracle(site):
    """int64 [H, W]: the exact squared distance to the nearest True of `site`, by the separable minimum: per column all
    pairs, then per row all pairs. 2^62 where there is no site."""
    site = np.asarray(site, dtype=bool)
    H, W = site.shape
    INF = np.int64(1) << 62
    ys = np.arange(H, dtype=np.int64)
    dy2 = (ys[:, None] - ys[None, :]) ** 2                            # [y, y']
    g2 = np.empty((H, W), dtype=np.int64)
    for x in range(W):
        g2[:, x] = np.where(site[None, :, x], dy2, INF).min(axis=1)
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                            # [x, x']
    out = np.empty((H, W), dtype=np.int64)
    for y in range(H):
        out[y] = np.minimum(g2[y][None, :] + dx2, INF).min(axis=1)
    return out


def brute_oracle(site):
    """(d2 int64 [H, W], nearest int64 [H, W]): all pixels x all sites; argmin over the sites in linear-index order, so the
    first of several nearest sites (the smallest index) wins. (2^62, -1) without a site. For small maps."""
    site = np.asarray(site, dtype=bool)
    H, W = site.shape
    sy, sx = np.nonzero(site)                                         # row-major: ascending linear index
    if len(sy) == 0:
        return np.full((H, W), np.int64(1) << 62), np.full((H, W), -1, dtype=np.int64)
    yy, xx = np.indices((H, W))
    d2 = np.empty((H, W), dtype=np.int64)
    near = np.empty((H, W), dtype=np.int64)
    for y in range(H):                                                # one row of pixels at a time: [W, sites]
        d = (y - sy[None, :]).astype(np.int64) ** 2 + (xx[y][:, None] - sx[None, :]).astype(np.int64) ** 2
        j = d.argmin(axis=1)
        d2[y] = d[np.arange(W), j]
        near[y] = sy[j] * W + sx[j]
    return d2, near


def nearest_oracle(site, max_distance=None):
    """(d2 int32, nearest int32) as the device returns them."""
    d2, near = brute_oracle(site)
    d2 = cap(d2, max_distance)
    return d2, np.where(d2 == FAR, -1, near).astype(np.int32)


def void_band_oracle(mask, width, void_value=255, ignore_value=255):
    mask = np.asarray(mask, dtype=np.uint8)
    d2 = dist_oracle(sites_oracle(mask, "edge", ignore_value))
    return np.where(d2 <= int(width) ** 2, np.uint8(void_value), mask).astype(np.uint8)


def expand_labels_oracle(labels, distance):
    labels = np.asarray(labels, dtype=np.int32)
    d2, near = brute_oracle(labels != 0)
    grown = labels.ravel()[np.maximum(near, 0)]
    return np.where((labels == 0) & (d2 <= int(distance) ** 2), grown, labels).astype(np.int32)


def boundary_counts_oracle(pred, gt, distance, num_classes, void_value=255):
    """int64 [K, 3] = (|P_c & G_c|, |P_c|, |G_c|) over the pixels with gt != void_value."""
    pred, gt = np.asarray(pred, dtype=np.uint8), np.asarray(gt, dtype=np.uint8)
    r2 = int(distance) ** 2
    near_p = dist_oracle(sites_oracle(pred, "edge", None)) <= r2
    near_g = dist_oracle(sites_oracle(gt, "edge", void_value)) <= r2
    live = np.ones(gt.shape, dtype=bool) if void_value is None else gt != void_value
    out = np.zeros((num_classes, 3), dtype=np.int64)
    for c in range(num_classes):
        P, G = live & near_p & (pred == c), live & near_g & (gt == c)
        out[c] = (int((P & G).sum()), int(P.sum()), int(G.sum()))
    return out


def striped_random(H, W, fill, seed):
    """Random foreground at `fill`, three classes in adjacent 37-pixel stripes (tests/test_score_gpu.py's maps)."""
    rng = np.random.default_rng(seed)
    cls = (1 + (np.arange(W) // 37) % 3).astype(np.uint8)
    return (rng.random((H, W)) < fill).astype(np.uint8) * cls[None, :]


def void_map(H, W, seed, share=0.1):
    """bool [H, W]: True on `share` of the pixels."""
    return np.random.default_rng(seed).random((H, W)) < share
