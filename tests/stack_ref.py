"""Numpy restatements of insar_unet_ca_amd/stack.py on csrc/stack.hip (push, shift, summary, series, the host derivations)
and the deterministic inputs of tests/test_stack_host.py and tests/test_stack_gpu.py. The state is two uint64 arrays
[words, H, W]: date t is bit t & 63 of plane t >> 6. Everything is defined by scans over the dates, vectorised over pixels;
tests/test_stack_host.py pins it against a per-pixel Python loop."""
import numpy as np

PLANES = ("n_valid", "n_hit", "longest_run", "run_start", "first_hit", "last_hit", "known", "persistent")
RULE = dict(min_hits=3, min_run=2, min_valid=4, min_fraction=(1, 4))
SERIES_FIELDS = ("area", "hits", "valids", "observed", "active", "onset", "last_active", "n_active", "longest_active_run")
U1 = np.uint64(1)


def empty_state(words, H, W):
    return np.zeros((words, H, W), dtype=np.uint64), np.zeros((words, H, W), dtype=np.uint64)


def get_bit(planes, t):
    return ((planes[t >> 6] >> np.uint64(t & 63)) & U1).astype(bool)


def set_bit(planes, t, b):
    m = U1 << np.uint64(t & 63)
    planes[t >> 6] = np.where(b, planes[t >> 6] | m, planes[t >> 6] & ~m)


def in_classes(mask, classes):
    cs = [classes] if isinstance(classes, (int, np.integer)) else list(classes)
    return np.isin(mask, np.asarray(cs, dtype=np.uint8))


def push_ref(hit, valid, mask, t, *, valid_in=None, conf=None, min_conf=0.0, classes=1, ignore=255):
    """New (hit, valid) with dates t .. t + n - 1 written from mask [n, H, W] (or [H, W])."""
    hit, valid = hit.copy(), valid.copy()
    mask = mask[None] if mask.ndim == 2 else mask
    valid_in = None if valid_in is None else (valid_in[None] if valid_in.ndim == 2 else valid_in)
    conf = None if conf is None else (conf[None] if conf.ndim == 2 else conf)
    for i in range(mask.shape[0]):
        v = np.ones(mask[i].shape, dtype=bool) if ignore is None else mask[i] != ignore
        if valid_in is not None:
            v &= valid_in[i] != 0
        h = v & in_classes(mask[i], classes)
        if conf is not None:
            with np.errstate(invalid="ignore"):
                h &= conf[i] >= np.float32(min_conf)               # a NaN compares false
        set_bit(valid, t + i, v)
        set_bit(hit, t + i, h)
    return hit, valid


def shift_ref(hit, valid, k):
    T = 64 * hit.shape[0]
    out = []
    for planes in (hit, valid):
        new = np.zeros_like(planes)
        for t in range(max(0, T - k)):
            set_bit(new, t, get_bit(planes, t + k))
        out.append(new)
    return out[0], out[1]


def scan_ref(hit_at, valid_at, dates, shape):
    """The one scan: `hit_at(t)`, `valid_at(t)` give bool arrays of `shape`; dates without the valid bit are skipped."""
    z = lambda v: np.full(shape, v, dtype=np.int64)
    n_valid, n_hit, best, best_start, cur, cur_start, first, last = z(0), z(0), z(0), z(-1), z(0), z(-1), z(-1), z(-1)
    for t in dates:
        v = valid_at(t)
        h = hit_at(t) & v
        miss = v & ~h
        n_valid += v
        n_hit += h
        cur_start = np.where(h & (cur == 0), t, cur_start)
        cur = cur + h
        better = cur > best
        best, best_start = np.where(better, cur, best), np.where(better, cur_start, best_start)
        cur, cur_start = np.where(miss, 0, cur), np.where(miss, -1, cur_start)
        first = np.where(h & (first < 0), t, first)
        last = np.where(h, t, last)
    return dict(n_valid=n_valid, n_hit=n_hit, longest_run=best, run_start=best_start, first_hit=first, last_hit=last)


def summary_ref(hit, valid, t0, t1, *, min_hits=1, min_run=1, min_valid=1, min_fraction=(0, 1)):
    s = scan_ref(lambda t: get_bit(hit, t), lambda t: get_bit(valid, t), range(t0, t1), hit.shape[1:])
    num, den = min_fraction
    known = s["n_valid"] >= min_valid
    pers = known & (s["n_hit"] >= min_hits) & (s["longest_run"] >= min_run) & (s["n_hit"] * den >= num * s["n_valid"])
    out = {k: v.astype(np.int16) for k, v in s.items()}
    out["known"], out["persistent"] = known.astype(np.uint8), pers.astype(np.uint8)
    return out


def derive_ref(area, hits, valids, active_fraction=(1, 2), t0=0):
    num, den = active_fraction
    observed = 2 * valids >= area[:, None]
    active = (valids > 0) & (hits * den >= num * valids)
    nt = hits.shape[1]
    s = scan_ref(lambda t: active[:, t - t0], lambda t: observed[:, t - t0], range(t0, t0 + nt), (hits.shape[0],))
    return dict(observed=observed, active=active, onset=s["first_hit"], last_active=s["last_hit"], n_active=s["n_hit"],
                longest_active_run=s["longest_run"])


def series_ref(hit, valid, labels, *, max_regions=65536, count=None, t0=0, t1=None, active_fraction=(1, 2)):
    t1 = 64 * hit.shape[0] if t1 is None else t1
    N = max_regions if count is None else count
    flat = labels.ravel().astype(np.int64)
    inside = (flat >= 1) & (flat <= max_regions)
    idx = flat[inside]
    area = np.bincount(idx, minlength=max_regions + 1)[1:].astype(np.int64)
    hits = np.zeros((max_regions, t1 - t0), dtype=np.int64)
    valids = np.zeros((max_regions, t1 - t0), dtype=np.int64)
    for t in range(t0, t1):
        v = get_bit(valid, t).ravel()[inside]
        h = get_bit(hit, t).ravel()[inside] & v
        valids[:, t - t0] = np.bincount(idx, weights=v, minlength=max_regions + 1)[1:]
        hits[:, t - t0] = np.bincount(idx, weights=h, minlength=max_regions + 1)[1:]
    out = dict(area=area[:N], hits=hits[:N], valids=valids[:N], out_of_range=int((flat > max_regions).sum()))
    out.update(derive_ref(out["area"], out["hits"], out["valids"], active_fraction, t0))
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------
def random_inputs(H, W, n, seed, values=(0, 1, 1, 1, 2, 3, 200, 255, 7)):
    """n dates of class maps over `values`, a validity map (10 % zeros) and confidences on a grid of sixteenths with NaN."""
    rng = np.random.default_rng(seed)
    mask = np.asarray(values, dtype=np.uint8)[rng.integers(0, len(values), size=(n, H, W))]
    valid_in = (rng.random((n, H, W)) >= 0.1).astype(np.uint8) * np.uint8(3)
    conf = (rng.integers(0, 17, size=(n, H, W)) / 16.0).astype(np.float32)            # many equal min_conf = 0.5 exactly
    conf[rng.random((n, H, W)) < 0.02] = np.nan
    return mask, valid_in, conf


def hard_bits(H, W, T, seed):
    """Intended hit / valid bits bool [T, H, W] with the hard cases planted at the first 240 pixels and blobs of persistent
    detections; needs H * W >= 2000 and T >= 131."""
    assert H * W >= 2000 and T >= 131
    rng = np.random.default_rng(seed)
    valid = rng.random((T, H, W)) < 0.85
    yy, xx = np.mgrid[0:H, 0:W]
    blob = np.zeros((H, W), dtype=bool)
    for _ in range(25):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(3, 12)
        blob |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    since = rng.integers(0, T // 2, size=(H, W))                   # each pixel of a blob starts at its own date
    hit = valid & ((rng.random((T, H, W)) < 0.08) | (blob[None] & (np.arange(T)[:, None, None] >= since[None]) & (rng.random((T, H, W)) < 0.9)))
    hf, vf = hit.reshape(T, -1), valid.reshape(T, -1)

    def plant(lo, hi, hits, invalid=()):
        vf[:, lo:hi] = True
        hf[:, lo:hi] = False
        hf[list(hits), lo:hi] = True
        vf[list(invalid), lo:hi] = False
        hf[list(invalid), lo:hi] = False

    plant(0, 150, [10, 11, 13, 14, 15], invalid=[12])             # the longest run bridges an unobserved date
    plant(150, 180, [20, 21, 22, 40, 41, 42])                     # two runs of the longest length: the earlier one counts
    vf[:, 180:190] = False                                         # never observed
    hf[:, 180:190] = False
    vf[:, 190:200] = True                                          # every date observed, 190..194 every date a hit
    hf[:, 190:195] = True
    plant(200, 220, range(60, 69))                                 # a run across bit 63 -> 64
    plant(220, 240, range(125, 131))                               # and across 127 -> 128
    return hit, valid


def inputs_from_bits(hit, valid, seed, min_conf=0.5):
    """Class maps, validity maps and confidences that push_ref(classes=1, ignore=255, min_conf) turns into exactly these
    bits, by every route: a miss is another class, a low or NaN confidence; unobserved is `ignore` or valid_in = 0."""
    rng = np.random.default_rng(seed)
    route = rng.integers(0, 3, size=hit.shape)
    mask = np.where(hit, 1, np.where(route == 0, 0, 1)).astype(np.uint8)
    conf = np.where(hit, np.where(route == 0, min_conf, 0.75), np.where(route == 1, 0.25, np.nan)).astype(np.float32)
    conf[~hit & (route == 0)] = 0.9                                # the class decides there
    valid_in = np.ones(hit.shape, dtype=np.uint8)
    mask[~valid & (route == 0)] = 255
    valid_in[~valid & (route != 0)] = 0
    mask[~valid & (route == 2)] = 1                                # a detection under valid_in = 0 is no hit
    conf[~valid & (route == 2)] = 1.0
    return mask, valid_in, conf


_HARD = {}


def hard_stack(H=200, W=264, T=131, seed=11):
    """(mask, valid_in, conf, hit planes, valid planes) of the hard stack, built once per shape; asserts the hard cases."""
    key = (H, W, T, seed)
    if key in _HARD:
        return _HARD[key]
    hb, vb = hard_bits(H, W, T, seed)
    mask, valid_in, conf = inputs_from_bits(hb, vb, seed + 1)
    words = (T + 63) // 64
    hit, valid = push_ref(*empty_state(words, H, W), mask, 0, valid_in=valid_in, conf=conf, min_conf=0.5)
    for t in (0, 12, 63, 64, 127, 128, T - 1):
        assert np.array_equal(get_bit(hit, t), hb[t]) and np.array_equal(get_bit(valid, t), vb[t]), t
    s = summary_ref(hit, valid, 0, T, **RULE)
    broken = scan_ref(lambda t: hb[t], lambda t: np.ones_like(vb[t]), range(T), (H, W))          # unobserved dates break runs
    assert int((s["longest_run"] > broken["longest_run"]).sum()) >= 100
    last_wins = _scan_ties_last(hb, vb)
    assert int(((last_wins != s["run_start"]) & (s["longest_run"] > 0)).sum()) >= 10              # two runs of equal longest length
    assert int((s["n_valid"] == 0).sum()) >= 10 and int((s["n_valid"] == T).sum()) >= 10
    f = s["run_start"].ravel().astype(int), s["longest_run"].ravel().astype(int)
    assert ((f[0] <= 63) & (f[0] + f[1] > 64)).sum() >= 20 and ((f[0] <= 127) & (f[0] + f[1] > 128)).sum() >= 20
    assert int((s["known"] == 0).sum()) >= 10 and int((s["persistent"] == 1).sum()) >= 200 and int((s["persistent"] == 0).sum()) >= 200
    assert np.isnan(conf).any() and (conf == 0.5).any() and (mask == 255).any() and (valid_in == 0).any()
    _HARD[key] = (mask, valid_in, conf, hit, valid)
    return _HARD[key]


def _scan_ties_last(hb, vb):
    """run_start where the LATEST of several longest runs wins: differs from the scan's exactly where there is a tie."""
    T, shape = hb.shape[0], hb.shape[1:]
    best, best_start, cur, cur_start = (np.zeros(shape, dtype=np.int64), np.full(shape, -1, dtype=np.int64),
                                        np.zeros(shape, dtype=np.int64), np.full(shape, -1, dtype=np.int64))
    for t in range(T):
        h, miss = hb[t] & vb[t], vb[t] & ~hb[t]
        cur_start = np.where(h & (cur == 0), t, cur_start)
        cur = cur + h
        better = (cur >= best) & (cur > 0)
        best, best_start = np.where(better, cur, best), np.where(better, cur_start, best_start)
        cur, cur_start = np.where(miss, 0, cur), np.where(miss, -1, cur_start)
    return best_start


def series_labels(H, W, seed, max_regions=40):
    """Random rectangular patches of ids 1..max_regions + 5 over background, a band of negative labels; asserts that ids above
    max_regions and negative ids are present."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), dtype=np.int32)
    for _ in range(150):
        y, x = rng.integers(0, H), rng.integers(0, W)
        lab[y:y + rng.integers(1, 23), x:x + rng.integers(1, 23)] = rng.integers(1, max_regions + 6)
    lab[H // 2, : W // 2] = -3
    lab[0, 0] = np.iinfo(np.int32).min
    lab[0, 1:3] = np.iinfo(np.int32).max
    assert (lab > max_regions).sum() > 20 and (lab < 0).sum() > 1 and (lab == 0).sum() > 0
    return lab
