"""numpy restatement of csrc/crops.hip, on Python-int aug_hash64 (insar_unet_ca_amd/augment.py): the cells by reshape-sum,
the table by cumsum, the draw as include/insar_hip.h states it, the gather by slicing. Everything is integer (the image
normalisation is the float32 arithmetic of insar_scene_gather), so the kernels are compared with it bitwise."""
import numpy as np

from insar_unet_ca_amd.augment import aug_hash64


def cells(labels: np.ndarray, K: int, g: int) -> np.ndarray:
    """int64 [K + 1, Hc, Wc]: pixels per cell and plane; plane K = void (255 and every other label >= K)."""
    H, W = labels.shape
    Hc, Wc = H // g, W // g
    lab = labels[:Hc * g, :Wc * g].astype(np.int64)
    out = np.zeros((K + 1, Hc, Wc), dtype=np.int64)
    for p in range(K + 1):
        hit = (lab == p) if p < K else (lab >= K)
        out[p] = hit.reshape(Hc, g, Wc, g).sum(axis=(1, 3))
    return out


def cell_table(labels: np.ndarray, K: int, g: int) -> np.ndarray:
    """int32 [K + 1, Hc + 1, Wc + 1]: what insar_crops_cells writes (row 0 and column 0 zero)."""
    c = cells(labels, K, g)
    out = np.zeros((K + 1, c.shape[1] + 1, c.shape[2] + 1), dtype=np.int32)
    out[:, 1:, 1:] = c
    return out


def sat(labels: np.ndarray, K: int, g: int) -> np.ndarray:
    """int32 [K + 1, Hc + 1, Wc + 1]: the exclusive 2-D prefix sums of the cells."""
    t = cell_table(labels, K, g).astype(np.int64)
    t = t.cumsum(axis=1).cumsum(axis=2)
    assert t.max() < 2 ** 31
    return t.astype(np.int32)


def rect(table: np.ndarray, p: int, a0: int, b0: int, n: int) -> int:
    """Pixels of plane p in the n x n cells from cell (a0, b0): four lookups."""
    t = table[p]
    return int(t[a0 + n, b0 + n]) - int(t[a0, b0 + n]) - int(t[a0 + n, b0]) + int(t[a0, b0])


def counts(table: np.ndarray, origins: np.ndarray, T: int, g: int) -> np.ndarray:
    """int32 [n, K + 1]: what CropIndex.counts returns."""
    return np.array([[rect(table, p, int(y) // g, int(x) // g, T // g) for p in range(table.shape[0])] for y, x in origins],
                    dtype=np.int32).reshape(len(origins), table.shape[0])


def draw(key: int, n: int, K: int, tries: int, cum, min_count: int, max_void: int, T: int, g: int, H: int, W: int,
         table: np.ndarray):
    """-> (origins int32 [n, 2], info int32 [n, 4]) of insar_crops_draw."""
    cum = np.asarray(cum, dtype=np.float32)
    Hc, Wc, tg = H // g, W // g, T // g
    ny, nx = Hc - tg + 1, Wc - tg + 1
    origins = np.zeros((n, 2), dtype=np.int32)
    info = np.zeros((n, 4), dtype=np.int32)
    for s in range(n):
        b = 65 * s
        u = np.float32(aug_hash64(key, b) >> 40) * np.float32(2.0 ** -24)
        cls = K - 1
        for c in range(K):
            if u < cum[c]:
                cls = c
                break
        tr = []
        for t in range(tries):
            r = aug_hash64(key, b + 1 + t)
            cy, cx = ((r >> 32) * ny) >> 32, ((r & 0xffffffff) * nx) >> 32
            tr.append((cy, cx, rect(table, cls, cy, cx, tg), rect(table, K, cy, cx, tg)))
        accepted = [t for t, (_, _, cnt, vd) in enumerate(tr) if cnt >= min_count and vd <= max_void]
        if accepted:
            win, acc = accepted[0], accepted[0]
        else:
            capped = [t for t, (_, _, _, vd) in enumerate(tr) if vd <= max_void]
            if capped:
                win = max(capped, key=lambda t: (tr[t][2], -t))
            else:
                win = min(range(tries), key=lambda t: (tr[t][3], t))
            acc = -1
        cy, cx, cnt, vd = tr[win]
        origins[s] = (cy * g, cx * g)
        info[s] = (cls, acc, cnt, vd)
    return origins, info


def normalise(tile: np.ndarray) -> np.ndarray:
    """insar_scene_gather's arithmetic: uint8 v -> (v / 255 - 0.5) / 0.5 in float32, each step rounded; float32 copied."""
    if tile.dtype == np.float32:
        return tile.copy()
    x = tile.astype(np.float32) / np.float32(255.0)
    return (x - np.float32(0.5)) / np.float32(0.5)


def gather(scene: np.ndarray, labels: np.ndarray, origins: np.ndarray, T: int, mask_dtype=np.int64):
    """-> (images float32 [n, 1, T, T], masks [n, T, T])."""
    images = np.stack([normalise(scene[y:y + T, x:x + T]) for y, x in origins])[:, None]
    masks = np.stack([labels[y:y + T, x:x + T] for y, x in origins]).astype(mask_dtype)
    return images.astype(np.float32), masks
