"""Host-only: the numpy restatement of tests/stack_ref.py pinned against a plain per-pixel Python loop, the argument checks of
insar_unet_ca_amd/stack.py and of the entry points of csrc/stack.hip (all of which come before the device is touched), the
table arithmetic, the bindings, the host derivations and the state round trip."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from insar_unet_ca_amd import _lib, stack
from insar_unet_ca_amd._lib import InsarError
from tests import stack_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("insar_stack_push", "insar_stack_shift", "insar_stack_summary", "insar_stack_series_bytes", "insar_stack_series_clear",
               "insar_stack_series")


# ---- the restatement against a pixel loop ---------------------------------------------------------------------------------
def loop_scan(hits, valids, t0):
    """One pixel (or one site): lists of bools over the window's dates."""
    n_valid = n_hit = best = cur = 0
    best_start = cur_start = first = last = -1
    for i, (h, v) in enumerate(zip(hits, valids)):
        if not v:
            continue                                              # a missing observation neither breaks nor extends a run
        n_valid += 1
        if h:
            n_hit += 1
            if cur == 0:
                cur_start = t0 + i
            cur += 1
            if cur > best:
                best, best_start = cur, cur_start
            if first < 0:
                first = t0 + i
            last = t0 + i
        else:
            cur, cur_start = 0, -1
    return dict(n_valid=n_valid, n_hit=n_hit, longest_run=best, run_start=best_start, first_hit=first, last_hit=last)


def test_restatement_equals_a_pixel_loop():
    H, W, T, words = 9, 13, 130, 3
    mask, valid_in, conf = ref.random_inputs(H, W, T, 5)
    classes, ignore, min_conf = (1, 3, 200), 7, 0.5
    hit, valid = ref.push_ref(*ref.empty_state(words, H, W), mask, 0, valid_in=valid_in, conf=conf, min_conf=min_conf, classes=classes,
                              ignore=ignore)
    # push: bit by bit from the inputs
    hb = np.zeros((64 * words, H, W), dtype=bool)
    vb = np.zeros((64 * words, H, W), dtype=bool)
    for t in range(T):
        for y in range(H):
            for x in range(W):
                m, c = int(mask[t, y, x]), float(conf[t, y, x])
                vb[t, y, x] = m != ignore and valid_in[t, y, x] != 0
                hb[t, y, x] = vb[t, y, x] and m in classes and (not math.isnan(c)) and c >= min_conf
    for t in range(64 * words):
        assert np.array_equal(ref.get_bit(hit, t), hb[t]) and np.array_equal(ref.get_bit(valid, t), vb[t]), t
    assert hb[:T].any() and (vb[:T] & ~hb[:T]).any() and (~vb[:T]).any() and not vb[T:].any()
    # an overwrite touches its own bits only
    h2, v2 = ref.push_ref(hit, valid, mask[5:8], 62, classes=2, ignore=None)
    for t in range(64 * words):
        if 62 <= t < 65:
            assert ref.get_bit(v2, t).all() and np.array_equal(ref.get_bit(h2, t), mask[5 + t - 62] == 2)
        else:
            assert np.array_equal(ref.get_bit(h2, t), hb[t]) and np.array_equal(ref.get_bit(v2, t), vb[t])
    # summary, three windows
    for t0, t1, rule in ((0, T, ref.RULE), (60, 70, dict(min_hits=2, min_run=2, min_valid=3, min_fraction=(1, 3))), (17, 17, dict(min_valid=0, min_hits=0, min_run=0))):
        got = ref.summary_ref(hit, valid, t0, t1, **rule)
        r = {**dict(min_hits=1, min_run=1, min_valid=1, min_fraction=(0, 1)), **rule}
        for y in range(H):
            for x in range(W):
                s = loop_scan(hb[t0:t1, y, x], vb[t0:t1, y, x], t0)
                for k, v in s.items():
                    assert int(got[k][y, x]) == v, (t0, t1, y, x, k)
                known = s["n_valid"] >= r["min_valid"]
                pers = (known and s["n_hit"] >= r["min_hits"] and s["longest_run"] >= r["min_run"]
                        and s["n_hit"] * r["min_fraction"][1] >= r["min_fraction"][0] * s["n_valid"])
                assert int(got["known"][y, x]) == known and int(got["persistent"][y, x]) == pers
        assert got["n_hit"].dtype == np.int16 and got["known"].dtype == np.uint8
    # shift
    for k in (0, 1, 63, 64, 65, 191, 192, 500):
        hs, vs = ref.shift_ref(hit, valid, k)
        for t in range(64 * words):
            want_h = hb[t + k] if t + k < 64 * words else np.zeros((H, W), dtype=bool)
            want_v = vb[t + k] if t + k < 64 * words else np.zeros((H, W), dtype=bool)
            assert np.array_equal(ref.get_bit(hs, t), want_h) and np.array_equal(ref.get_bit(vs, t), want_v), (k, t)
    # series and the derivations
    rng = np.random.default_rng(9)
    labels = rng.integers(-1, 9, size=(H, W)).astype(np.int32)
    labels[labels == 2] = 0
    R, t0, t1 = 6, 3, 120
    got = ref.series_ref(hit, valid, labels, max_regions=R, t0=t0, t1=t1, active_fraction=(1, 3))
    assert got["out_of_range"] == int((labels > R).sum()) > 0 and got["area"][1] == 0
    for l in range(1, R + 1):
        ys, xs = np.nonzero(labels == l)
        assert got["area"][l - 1] == len(ys)
        hits = [sum(int(hb[t, y, x]) for y, x in zip(ys, xs)) for t in range(t0, t1)]
        valids = [sum(int(vb[t, y, x]) for y, x in zip(ys, xs)) for t in range(t0, t1)]
        assert got["hits"][l - 1].tolist() == hits and got["valids"][l - 1].tolist() == valids
        observed = [2 * v >= len(ys) for v in valids]
        active = [v > 0 and 3 * h >= v for h, v in zip(hits, valids)]
        assert got["observed"][l - 1].tolist() == observed and got["active"][l - 1].tolist() == active
        s = loop_scan(active, observed, t0)
        assert (int(got["onset"][l - 1]), int(got["last_active"][l - 1]), int(got["n_active"][l - 1]), int(got["longest_active_run"][l - 1])) == \
            (s["first_hit"], s["last_hit"], s["n_hit"], s["longest_run"])


def test_the_hard_stack_reaches_the_hard_cases():
    mask, valid_in, conf, hit, valid = ref.hard_stack()           # asserts inside
    assert mask.shape == (131, 200, 264) and hit.shape == (3, 200, 264)
    ref.series_labels(200, 264, 21)


def test_the_package_scan_is_the_restatement():
    rng = np.random.default_rng(2)
    h, v = rng.random((50, 40)) < 0.5, rng.random((50, 40)) < 0.7
    got = stack.scan_runs(h, v, 7)
    want = ref.scan_ref(lambda t: h[:, t - 7], lambda t: v[:, t - 7], range(7, 47), (50,))
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_series_from_table_on_a_hand_made_table():
    R, nt = 3, 4
    raw = np.zeros(stack.series_bytes(R, nt), dtype=np.uint8)
    w = raw.view("<i4")
    w[0] = 5
    rows = w[4:4 + R * 9].reshape(R, 9)
    rows[0] = [10, 0, 6, 5, 1, 10, 10, 4, 10]                      # date 2 is seen on 4 of 10 pixels: not observed, it bridges
    rows[1] = [4, 0, 0, 0, 0, 4, 4, 4, 4]
    s = stack.series_from_table(raw, max_regions=R, n_dates=nt, count=2, t0=8, active_fraction=(1, 2))
    assert s["out_of_range"] == 5 and s["area"].tolist() == [10, 4] and s["hits"].shape == (2, 4) and s["hits"].dtype == np.int64
    assert s["observed"].tolist() == [[True, True, False, True], [True] * 4]
    assert s["active"].tolist() == [[False, True, True, False], [False] * 4]
    assert s["onset"].tolist() == [9, -1] and s["last_active"].tolist() == [9, -1] and s["n_active"].tolist() == [1, 0]
    assert s["longest_active_run"].tolist() == [1, 0] and (s["t0"], s["t1"]) == (8, 12)
    full = stack.series_from_table(raw, max_regions=R, n_dates=nt, count=None)
    assert full["area"].tolist() == [10, 4, 0] and full["valids"][2].tolist() == [0] * 4


# ---- argument checks: before anything touches the device ------------------------------------------------------------------
def _st(words=2):
    return stack.DetectionStack(6, 8, "cpu", words)


def test_construction_is_refused():
    for args, match in (((0, 8, "cpu"), "grid"), ((6, 8.0, "cpu"), "grid"), ((65536, 65536, "cpu"), "2\\^31"), ((6, 8, "cpu", 0), "words"),
                        ((6, 8, "cpu", 5), "words"), ((6, 8, "cpu", True), "words")):
        with pytest.raises(InsarError, match=match):
            stack.DetectionStack(*args)
    st = _st(4)
    assert st.hit.shape == (4, 6, 8) and st.hit.dtype == torch.int64 and st.valid.shape == (4, 6, 8) and st.n_dates == 0 and st.T == 256


@pytest.mark.parametrize("make,kw,match", [
    (lambda m: m.int(), {}, "dtype"),
    (lambda m: m.numpy(), {}, "torch tensor"),
    (lambda m: m[:, :7], {}, "shape"),
    (lambda m: m[None, None], {}, "shape"),
    (lambda m: torch.zeros(0, 6, 8, dtype=torch.uint8), {}, "shape"),
    (lambda m: torch.zeros(6, 16, dtype=torch.uint8)[:, ::2], {}, "contiguous"),
    (lambda m: m, {"valid": torch.zeros(2, 6, 8, dtype=torch.uint8)}, "as the mask"),
    (lambda m: m, {"valid": torch.zeros(6, 8)}, "valid dtype"),
    (lambda m: m, {"conf": torch.zeros(6, 8, dtype=torch.float64)}, "conf dtype"),
    (lambda m: m, {"conf": torch.zeros(8, 6).t()}, "contiguous"),
    (lambda m: m, {"t": -1}, "beyond"),
    (lambda m: m, {"t": 128}, "beyond"),
    (lambda m: m, {"t": 1.0}, "beyond"),
    (lambda m: torch.zeros(5, 6, 8, dtype=torch.uint8), {"t": 124}, "beyond"),
    (lambda m: m, {"classes": 256}, "classes"),
    (lambda m: m, {"classes": [1, -1]}, "classes"),
    (lambda m: m, {"classes": []}, "classes"),
    (lambda m: m, {"classes": 1.5}, "classes"),
    (lambda m: m, {"ignore": 256}, "ignore"),
    (lambda m: m, {"ignore": -2}, "ignore"),
    (lambda m: m, {"min_conf": math.nan}, "min_conf"),
    (lambda m: m, {"min_conf": math.inf}, "min_conf"),
    (lambda m: m, {"min_conf": "x"}, "min_conf"),
    (lambda m: m, {}, "ROCm"),                                     # every other check passed: the host tensor is refused last
])
def test_push_checks_raise_on_the_host(make, kw, match):
    with pytest.raises(InsarError, match=match):
        _st().push(make(torch.zeros(6, 8, dtype=torch.uint8)), **kw)


@pytest.mark.parametrize("kw,match", [
    ({"t0": -1}, "window"), ({"t0": 5, "t1": 4}, "window"), ({"t1": 129}, "window"), ({"t1": 2.0}, "window"),
    ({"min_hits": -1}, "min_hits"), ({"min_run": 40000}, "min_run"), ({"min_valid": 1.5}, "min_valid"),
    ({"min_fraction": (2, 1)}, "min_fraction"), ({"min_fraction": (0, 0)}, "min_fraction"), ({"min_fraction": 0.5}, "min_fraction"),
    ({"min_fraction": (-1, 2)}, "min_fraction"), ({"min_fraction": (1, 1 << 31)}, "min_fraction"), ({"min_fraction": (0.5, 1)}, "min_fraction"),
    ({"want": ()}, "want"), ({"want": ("n_hit", "median")}, "want"), ({"want": ("n_hit", "n_hit")}, "want"),
    ({}, "ROCm"),
])
def test_summary_checks_raise_on_the_host(kw, match):
    with pytest.raises(InsarError, match=match):
        _st().summary(**kw)


def test_shift_checks_raise_on_the_host():
    for k, match in ((-1, "k="), (1.0, "k="), (True, "k="), (1 << 31, "k="), (3, "ROCm")):
        with pytest.raises(InsarError, match=match):
            _st().shift(k)


@pytest.mark.parametrize("make,kw,match", [
    (lambda l: l.long(), {}, "int32"),
    (lambda l: l[:, :7], {}, "int32 \\[6, 8\\]"),
    (lambda l: l.numpy(), {}, "torch tensor"),
    (lambda l: torch.zeros(6, 16, dtype=torch.int32)[:, ::2], {}, "contiguous"),
    (lambda l: l, {"max_regions": 0}, "max_regions"),
    (lambda l: l, {"max_regions": (1 << 24) + 1}, "max_regions"),
    (lambda l: l, {"max_regions": 4, "count": 5}, "count"),
    (lambda l: l, {"count": -1}, "count"),
    (lambda l: l, {"t0": 3, "t1": 2}, "window"),
    (lambda l: l, {"t1": 200}, "window"),
    (lambda l: l, {"active_fraction": (3, 2)}, "active_fraction"),
    (lambda l: l, {"active_fraction": None}, "active_fraction"),
    (lambda l: l, {}, "ROCm"),
])
def test_series_checks_raise_on_the_host(make, kw, match):
    with pytest.raises(InsarError, match=match):
        stack.site_series(_st(), make(torch.zeros(6, 8, dtype=torch.int32)), **kw)
    with pytest.raises(InsarError, match="DetectionStack"):
        stack.site_series(None, torch.zeros(6, 8, dtype=torch.int32))


def test_a_scratch_of_the_wrong_size_is_refused():
    st, labels = _st(), torch.zeros(6, 8, dtype=torch.int32)
    st.n_dates = 10
    stub = lambda R, n, nbytes: types.SimpleNamespace(max_regions=R, n_dates=n, table=torch.zeros(nbytes, dtype=torch.uint8))
    want = stack.series_bytes(16, 10)
    for sc in (stub(8, 10, stack.series_bytes(8, 10)), stub(16, 9, stack.series_bytes(16, 9)), stub(16, 10, want - 16)):
        with pytest.raises(InsarError, match="scratch"):
            stack.site_series(st, labels, max_regions=16, scratch=sc)
    with pytest.raises(InsarError, match="ROCm"):
        stack.site_series(st, labels, max_regions=16, scratch=stub(16, 10, want))
    with pytest.raises(InsarError, match="16-byte aligned uint8"):
        stack.StackScratch("cpu", 16, 10, table=torch.zeros(want + 1, dtype=torch.uint8))


def test_follow_sites_and_detect_stack_refuse_on_the_host():
    import insar_unet_ca_amd as iu
    with pytest.raises(InsarError, match="DetectionStack"):
        stack.follow_sites(None)
    with pytest.raises(InsarError, match="max_regions"):
        stack.follow_sites(_st(), max_regions=0)
    with pytest.raises(InsarError, match="active_fraction"):
        stack.follow_sites(_st(), active_fraction=(2, 1))
    with pytest.raises(InsarError, match="min_run"):
        stack.follow_sites(_st(), min_run=-1)
    with pytest.raises(InsarError, match="ROCm"):
        stack.follow_sites(_st())
    pred = iu.ScenePredictor(torch.nn.Conv2d(1, 2, 1), tile=32, overlap=8, batch=2)
    scene = np.zeros((64, 80), dtype=np.uint8)
    for scenes, kw, match in (([], {}, "0 scenes"), ([scene] * 257, {}, "257 scenes"), ([scene, scene[:, :64]], {}, "share one 2-D shape"),
                              ([scene[None]], {}, "share one 2-D shape"), (5, {}, "sequence"), ([scene] * 2, {"valids": [None]}, "validity maps"),
                              ([scene] * 65, {"words": 1}, "words"), ([scene], {"words": 5}, "words"),
                              ([scene[:16, :16]], {}, "tile")):
        with pytest.raises(InsarError, match=match):
            pred.detect_stack(scenes, **kw)


def test_entry_points_refuse_before_the_device():
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    push = lambda **o: _lib.call("insar_stack_push", *[{**dict(mask=p, vin=None, conf=None, mc=0.0, c0=2, c1=0, c2=0, c3=0, ign=255, n=1, t=0,
                                                               words=1, H=4, W=4, hit=p, valid=p, s=None), **o}[k]
                                                      for k in ("mask", "vin", "conf", "mc", "c0", "c1", "c2", "c3", "ign", "n", "t", "words", "H", "W",
                                                                "hit", "valid", "s")])
    for o, match in ((dict(mask=None), "null"), (dict(hit=None), "null"), (dict(valid=None), "null"), (dict(words=0), "words"),
                     (dict(words=5), "words"), (dict(H=0), "empty"), (dict(H=65536, W=65536), "2\\^31"), (dict(hit=p + 4), "aligned"),
                     (dict(n=0), "dates"), (dict(t=-1), "dates"), (dict(t=60, n=5), "dates"), (dict(ign=256), "ignore"),
                     (dict(mc=math.nan), "min_conf"), (dict(conf=p + 2), "aligned")):
        with pytest.raises(InsarError, match=match):
            push(**o)
    with pytest.raises(InsarError, match="negative"):
        _lib.call("insar_stack_shift", p, p, 1, 4, 4, -1, None)
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_stack_shift", None, p, 1, 4, 4, 1, None)
    summ = lambda **o: _lib.call("insar_stack_summary", *[{**dict(hit=p, valid=p, words=2, H=4, W=4, t0=0, t1=100, mh=1, mr=1, mv=1, num=0, den=1,
                                                                  a=p, b=None, c=None, d=None, e=None, f=None, g=None, h=None, s=None), **o}[k]
                                                         for k in ("hit", "valid", "words", "H", "W", "t0", "t1", "mh", "mr", "mv", "num", "den", "a",
                                                                   "b", "c", "d", "e", "f", "g", "h", "s")])
    for o, match in ((dict(hit=None), "null"), (dict(a=None), "every output"), (dict(t0=-1), "window"), (dict(t1=129), "window"),
                     (dict(t0=9, t1=8), "window"), (dict(mh=-1), "min_hits"), (dict(mr=32768), "min_run"), (dict(den=0), "fraction"),
                     (dict(num=2, den=1), "fraction"), (dict(num=-1), "fraction"), (dict(a=p + 1), "aligned"), (dict(words=9), "words")):
        with pytest.raises(InsarError, match=match):
            summ(**o)
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_stack_series_clear", None, 4, 10, None)
    with pytest.raises(InsarError, match="aligned"):
        _lib.call("insar_stack_series_clear", p + 8, 4, 10, None)
    with pytest.raises(InsarError, match="dates"):
        _lib.call("insar_stack_series_clear", p, 4, 257, None)
    ser = lambda **o: _lib.call("insar_stack_series", *[{**dict(hit=p, valid=p, words=1, labels=p, H=4, W=4, t0=0, t1=10, R=4, table=p, s=None), **o}[k]
                                                        for k in ("hit", "valid", "words", "labels", "H", "W", "t0", "t1", "R", "table", "s")])
    for o, match in ((dict(labels=None), "null"), (dict(table=None), "null"), (dict(valid=None), "null"), (dict(labels=p + 2), "aligned"),
                     (dict(table=p + 4), "aligned"), (dict(t1=65), "window"), (dict(R=0), "max_regions"), (dict(R=(1 << 24) + 1), "max_regions"),
                     (dict(W=0), "empty")):
        with pytest.raises(InsarError, match=match):
            ser(**o)


# ---- table arithmetic, bindings, state ------------------------------------------------------------------------------------
def test_series_bytes_is_host_arithmetic_and_monotone():
    assert stack.series_bytes(1, 0) == 32 and stack.series_bytes(1, 1) == 32 and stack.series_bytes(1, 2) == 48
    assert stack.series_bytes(65536, 64) == 16 + 4 * 65536 * 129
    assert stack.series_bytes(3, 7) == ((4 * (4 + 3 * 15) + 15) // 16) * 16
    assert stack.series_bytes(1 << 24, 256) == 16 + 4 * (1 << 24) * 513 > 1 << 35
    for R in (1, 2, 100, 65536):
        for n in (0, 1, 63, 64, 256):
            b = stack.series_bytes(R, n)
            assert b % 16 == 0 and b >= 4 * (stack.SERIES_HEADER + R * (1 + 2 * n))
            assert b >= stack.series_bytes(max(R - 1, 1), n) and b >= stack.series_bytes(R, max(n - 1, 0))
    for bad in ((0, 1), ((1 << 24) + 1, 1), (4, -1), (4, 257)):
        with pytest.raises(InsarError):
            stack.series_bytes(*bad)
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_stack_series_bytes", 4, 4, None)


def test_class_words():
    assert stack.class_words(1) == (2, 0, 0, 0) and stack.class_words(0) == (1, 0, 0, 0)
    assert stack.class_words([1, 3, 200]) == (0b1010, 0, 0, 1 << 8) and stack.class_words((63, 64, 255)) == (1 << 63, 1, 0, 1 << 63)
    assert stack.class_words(np.uint8(5)) == (32, 0, 0, 0)


def test_symbols_are_declared_exported_and_bound():
    assert _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert lib.insar_version() == 8
    header = open(os.path.join(ROOT, "include", "insar_hip.h")).read()
    assert re.search(r"#define INSAR_ABI_VERSION 8\b", header)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES and hasattr(lib, name)
    assert len(_lib._SIGNATURES["insar_stack_push"]) == 17 and len(_lib._SIGNATURES["insar_stack_summary"]) == 21
    import insar_unet_ca_amd as iu
    for name in ("DetectionStack", "StackScratch", "site_series", "follow_sites"):
        assert name in iu.__all__ and getattr(iu, name) is getattr(stack, name)
    assert callable(iu.ScenePredictor.detect_stack)
    assert "stack.hip" in open(os.path.join(ROOT, "insar_unet_ca_amd", "csrc", "Makefile")).read()


def test_state_dict_round_trip_on_the_host():
    a = _st(2)
    g = torch.Generator().manual_seed(1)
    a.hit.copy_(torch.randint(-(1 << 62), 1 << 62, (2, 6, 8), generator=g))
    a.valid.copy_(torch.randint(-(1 << 62), 1 << 62, (2, 6, 8), generator=g))
    a.n_dates = 77
    sd = a.state_dict()
    b = _st(2)
    b.load_state_dict({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()})
    assert torch.equal(b.hit, a.hit) and torch.equal(b.valid, a.valid) and b.n_dates == 77
    assert b.hit.data_ptr() != a.hit.data_ptr()
    for bad, match in (({}, "hit, valid and n_dates"), ({**sd, "hit": sd["hit"][:1]}, "int64 tensor"), ({**sd, "valid": sd["valid"].int()}, "int64 tensor"),
                       ({**sd, "n_dates": 129}, "n_dates"), ({**sd, "n_dates": 1.0}, "n_dates")):
        with pytest.raises(InsarError, match=match):
            _st(2).load_state_dict(bad)
