"""CPU restatement of insar_unet_ca_amd.sieve (a helper, not a test module): `label_all`, `adjacency` and `sieve` in numpy and
plain Python, written from the rule of DESIGN.md's "Sieving class maps" and not from the kernels. Components come from
scipy.ndimage.label per class, numbered by ascending first (smallest row-major) pixel index; keys are Python tuples
(area, -id). tests/test_sieve_host.py pins it on the prototype's findings."""
import numpy as np
from scipy import ndimage

STRUCTURE = {4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool), 8: np.ones((3, 3), dtype=bool)}


def table(min_area):
    """The 256 thresholds of an int (every class), a {class: int} dict (missing classes 0) or a sequence indexed by class."""
    T = np.zeros(256, dtype=np.int64)
    if isinstance(min_area, dict):
        for c, t in min_area.items():
            T[int(c)] = int(t)
    elif np.ndim(min_area) == 0:
        T[:] = int(min_area)
    else:
        T[:len(min_area)] = np.asarray(min_area, dtype=np.int64)
    return T


def label_all(mask, connectivity=8, void_value=255):
    """-> (labels int32 [H, W], area int64 [N + 1], cls int32 [N + 1]): the connected components over ALL classes, class 0
    included; void pixels carry label 0; ids 1..N by ascending smallest row-major pixel index. Entry 0 of the tables is 0."""
    m = np.asarray(mask, dtype=np.uint8)
    H, W = m.shape
    prov = np.zeros((H, W), dtype=np.int64)
    n_prov = 0
    for c in np.unique(m):
        if void_value is not None and c == void_value:
            continue
        lab, n = ndimage.label(m == c, structure=STRUCTURE[connectivity])
        prov = np.where(lab > 0, lab.astype(np.int64) + n_prov, prov)
        n_prov += n
    flat = prov.ravel()
    first = np.full(n_prov + 1, H * W, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(H * W, dtype=np.int64))
    order = np.argsort(first[1:], kind="stable")                  # ascending first pixel
    new_id = np.zeros(n_prov + 1, dtype=np.int32)
    new_id[order + 1] = np.arange(1, n_prov + 1, dtype=np.int32)
    labels = new_id[prov].astype(np.int32)
    area = np.bincount(labels.ravel(), minlength=n_prov + 1).astype(np.int64)
    area[0] = 0
    cls = np.zeros(n_prov + 1, dtype=np.int32)
    cls[1:] = m.ravel()[first[1:][order]]
    return labels, area, cls


def adjacency(labels):
    """-> dict(a, b int32, edges int64, count): every horizontally or vertically adjacent pixel pair whose labels a != b are
    both positive, counted under (min, max); sorted by (a, b)."""
    L = np.asarray(labels).astype(np.int64)
    p = np.concatenate([L[:, :-1].ravel(), L[:-1, :].ravel()])
    q = np.concatenate([L[:, 1:].ravel(), L[1:, :].ravel()])
    keep = (p != q) & (p > 0) & (q > 0)
    lo, hi = np.minimum(p[keep], q[keep]), np.maximum(p[keep], q[keep])
    if len(lo) == 0:
        z = np.zeros(0, dtype=np.int32)
        return {"a": z, "b": z.copy(), "edges": np.zeros(0, dtype=np.int64), "count": 0}
    pairs, counts = np.unique(np.stack([lo, hi], axis=1), axis=0, return_counts=True)
    return {"a": pairs[:, 0].astype(np.int32), "b": pairs[:, 1].astype(np.int32), "edges": counts.astype(np.int64),
            "count": int(len(counts))}


def sieve(mask, min_area, connectivity=8, void_value=255, max_rounds=64):
    """-> dict(mask, regions_in, absorbed, changed_pixels, rounds, converged, labels_in, root, changed, area, cls): the rule,
    round by round on a snapshot. `area` and `cls` are those of the input regions."""
    m = np.asarray(mask, dtype=np.uint8)
    T = table(min_area)
    labels, area0, cls = label_all(m, connectivity, void_value)
    N = len(area0) - 1
    adj = adjacency(labels)
    pa, pb = adj["a"].astype(np.int64), adj["b"].astype(np.int64)
    root = np.arange(N + 1, dtype=np.int64)
    area = area0.copy()
    rounds, converged = 0, False
    for _ in range(max_rounds):
        key = lambda u: (int(area[u]), -int(u))
        nbrs = {}
        for u, v in zip(root[pa], root[pb]):
            if u != v:
                nbrs.setdefault(int(u), set()).add(int(v))
                nbrs.setdefault(int(v), set()).add(int(u))
        best = {u: max(vs, key=key) for u, vs in nbrs.items() if area[u] < T[cls[u]]}
        nxt = {}
        for u, v in best.items():
            if best.get(v) == u and key(u) > key(v):
                continue                                          # the greater key of a mutual pair stays root
            nxt[u] = v
        if not nxt:
            converged = True
            break
        rounds += 1
        snapshot = area.copy()
        for u in nxt:
            r = u
            while r in nxt:
                r = nxt[r]
            area[r] += snapshot[u]
        for r in range(1, N + 1):
            x = int(root[r])
            while x in nxt:
                x = nxt[x]
            root[r] = x
    out = np.where(labels > 0, cls[root[labels]].astype(np.uint8), m).astype(np.uint8)
    changed = (out != m).astype(np.uint8)
    return {"mask": out, "regions_in": N, "absorbed": int((root[1:] != np.arange(1, N + 1)).sum()),
            "changed_pixels": int(changed.sum()), "rounds": rounds, "converged": converged, "labels_in": labels,
            "root": root.astype(np.int32), "changed": changed, "area": area0, "cls": cls}


def violations(res, min_area):
    """Pieces of a result that are below their class threshold and still have a neighbouring piece: the postcondition says
    there are none (where converged)."""
    T = table(min_area)
    root = res["root"].astype(np.int64)
    N = res["regions_in"]
    area = np.bincount(root[1:], weights=res["area"][1:], minlength=N + 1).astype(np.int64)
    adj = adjacency(res["labels_in"])
    u, v = root[adj["a"]], root[adj["b"]]
    has_nbr = np.zeros(N + 1, dtype=bool)
    has_nbr[u[u != v]] = True
    has_nbr[v[u != v]] = True
    pieces = np.flatnonzero(root == np.arange(N + 1))[1:]
    return [int(p) for p in pieces if area[p] < T[res["cls"][p]] and has_nbr[p]]


# ---- the maps of the prototype ------------------------------------------------------------------------------------------------
def blob_speckle(H, W, seed, classes=2, void=0.01):
    """Smooth blobs of `classes` classes with salt-and-pepper speckle and a share `void` of void (255) pixels."""
    rng = np.random.default_rng(seed)
    f = ndimage.uniform_filter(rng.random((H, W)), size=min(9, max(1, min(H, W))), mode="nearest")
    edges = np.quantile(f, np.linspace(0, 1, classes + 1)[1:-1]) if H * W > 1 else []
    m = np.digitize(f, edges).astype(np.uint8)
    flip = rng.random((H, W)) < 0.08
    m = np.where(flip, rng.integers(0, classes, size=(H, W)), m).astype(np.uint8)
    if void:
        m[rng.random((H, W)) < void] = 255
    return m


def strips(widths, first_class=0):
    """A 1-row map of strips of alternating classes first_class, 1 - first_class, ... with these widths."""
    return np.concatenate([np.full(w, (first_class + i) % 2, dtype=np.uint8) for i, w in enumerate(widths)])[None, :]


def squares(n=41):
    """Concentric alternating squares: ring k (Chebyshev distance k from the border) carries class k % 2."""
    y, x = np.mgrid[0:n, 0:n]
    return (np.minimum(np.minimum(y, x), np.minimum(n - 1 - y, n - 1 - x)) % 2).astype(np.uint8)


STRIPS_2 = ([5, 3, 4, 100], 10, 2)                                # widths, threshold for both classes, rounds
STRIPS_3 = ([7, 8, 1, 6, 2, 6, 7, 6, 8, 200], 40, 3)
SHAPES = [(1, 1), (1, 7), (5, 3), (33, 65), (64, 128), (97, 130)]
