"""CPU oracle of insar_unet_ca_amd.regions.label_regions, built on scipy.ndimage.label (a helper, not a test module):
label `mask == c` per class c >= 1 with the 4- or 8-structure after the min_conf threshold, drop components below min_area,
merge the classes and number the kept components by ascending first (smallest row-major) pixel index; statistics in int64 /
float64. tests/test_regions_host.py pins it against a brute-force flood fill."""
import numpy as np
from scipy import ndimage

CONF_SCALE = 1 << 30
STRUCTURE = {4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool), 8: np.ones((3, 3), dtype=bool)}


def quantise_conf(conf):
    """int64 llrint(clamp(conf, 0, 1) * 2^30) of a float32 field: the product is exact in float32 (a power of two), hence
    also in float64; np.rint rounds half to even like llrint."""
    c = np.clip(np.asarray(conf, dtype=np.float32), np.float32(0), np.float32(1)).astype(np.float64)
    return np.rint(c * CONF_SCALE).astype(np.int64)


def foreground(mask, conf=None, min_conf=0.0):
    """The class map with the sub-threshold pixels set to 0 (the comparison is made in float32, as on the device)."""
    m = np.asarray(mask, dtype=np.uint8)
    if conf is not None:
        m = np.where(np.asarray(conf, dtype=np.float32) >= np.float32(min_conf), m, 0).astype(np.uint8)
    return m


def regions_oracle(mask, conf=None, connectivity=8, min_area=1, min_conf=0.0):
    """-> dict(labels int32 [H, W], mask uint8 [H, W], count, regions) with regions a dict of arrays of length N: id, cls,
    area, y0, x0, y1, x1, cy, cx, root, sum_y, sum_x and, with conf, sum_conf (int64) and mean_conf."""
    m = foreground(mask, conf, min_conf)
    H, W = m.shape
    prov = np.zeros((H, W), dtype=np.int64)          # provisional component numbers 1.., all classes
    n_prov = 0
    for c in np.unique(m):
        if c == 0:
            continue
        lab, n = ndimage.label(m == c, structure=STRUCTURE[connectivity])
        prov = np.where(lab > 0, lab.astype(np.int64) + n_prov, prov)
        n_prov += n
    flat = prov.ravel()
    area = np.bincount(flat, minlength=n_prov + 1)[1:]
    first = np.full(n_prov + 1, H * W, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(H * W, dtype=np.int64))
    first = first[1:]
    kept = np.flatnonzero(area >= min_area)
    kept = kept[np.argsort(first[kept], kind="stable")]          # ascending root
    n = len(kept)
    new_id = np.zeros(n_prov + 1, dtype=np.int32)
    new_id[kept + 1] = np.arange(1, n + 1, dtype=np.int32)
    labels = new_id[prov].astype(np.int32)
    clean = np.where(labels > 0, m, 0).astype(np.uint8)

    lf = labels.ravel().astype(np.int64)
    yy, xx = np.divmod(np.arange(H * W, dtype=np.int64), W)

    def total(values):
        """Exact int64 sums per label: np.bincount adds in float64, so the values go in as two parts whose sums stay below
        2^53 (low 20 bits: < 2^20 * 2^31; the rest: < 2^11 * 2^31 for everything summed here)."""
        lo = np.bincount(lf, weights=(values & 0xFFFFF).astype(np.float64), minlength=n + 1)
        hi = np.bincount(lf, weights=(values >> 20).astype(np.float64), minlength=n + 1)
        return ((hi.astype(np.int64) << 20) + lo.astype(np.int64))[1:]

    boxes = ndimage.find_objects(labels, max_label=n)

    def extreme(axis, end):
        return np.array([getattr(b[axis], end) for b in boxes], dtype=np.int32).reshape(n)

    a = total(np.ones(H * W, dtype=np.int64))
    sy, sx = total(yy), total(xx)
    root = first[kept]
    reg = {"id": np.arange(1, n + 1, dtype=np.int32), "cls": m.ravel()[root].astype(np.int32), "area": a,
           "y0": extreme(0, "start"), "x0": extreme(1, "start"), "y1": extreme(0, "stop"), "x1": extreme(1, "stop"),
           "cy": sy.astype(np.float64) / a, "cx": sx.astype(np.float64) / a, "root": root, "sum_y": sy, "sum_x": sx}
    if conf is not None:
        sc = total(quantise_conf(conf).ravel())
        reg["sum_conf"] = sc
        reg["mean_conf"] = sc.astype(np.float64) / (a.astype(np.float64) * CONF_SCALE)
    return {"labels": labels, "mask": clean, "count": n, "regions": reg}
