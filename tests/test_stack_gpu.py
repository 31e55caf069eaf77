"""GPU: detections through a stack of dates (insar_unet_ca_amd/stack.py on csrc/stack.hip) against the numpy restatement of
tests/stack_ref.py (pinned against a pixel loop in tests/test_stack_host.py). Every comparison is bitwise.

Maps: 37 x 203 (odd: no 16-byte path), 1 x 1, 3 x 1025 (three pixels past three 1024-pixel passes) and 200 x 264 (a multiple
of four, 52 passes over several work-groups)."""
import numpy as np
import pytest
import torch

from tests import stack_ref as ref

pytestmark = pytest.mark.gpu
MAPS = [(37, 203), (1, 1), (3, 1025), (200, 264)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _state(st):
    torch.cuda.synchronize()
    return st.hit.cpu().numpy().view(np.uint64), st.valid.cpu().numpy().view(np.uint64)


def _assert_state(st, hit, valid, what=""):
    gh, gv = _state(st)
    for name, g, w in (("hit", gh, hit), ("valid", gv, valid)):
        bad = np.flatnonzero((g != w).reshape(-1))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:5]}: {g.reshape(-1)[bad[:5]]} vs {w.reshape(-1)[bad[:5]]}"


def _stack(dev, hit, valid, n_dates):
    import insar_unet_ca_amd as iu
    words, H, W = hit.shape
    st = iu.DetectionStack(H, W, dev, words)
    st.load_state_dict({"hit": torch.from_numpy(hit.view(np.int64)), "valid": torch.from_numpy(valid.view(np.int64)), "n_dates": n_dates})
    return st


def _assert_planes(got, want, what="", planes=ref.PLANES):
    assert set(got) == set(planes), what
    for p in planes:
        g = got[p].cpu().numpy()
        assert g.dtype == want[p].dtype and g.shape == want[p].shape, (what, p)
        bad = np.flatnonzero((g != want[p]).reshape(-1))
        assert bad.size == 0, f"{what}: {p} differs at {bad[:5]}: {g.reshape(-1)[bad[:5]]} vs {want[p].reshape(-1)[bad[:5]]}"


def _assert_series(got, want, what=""):
    assert got["out_of_range"] == want["out_of_range"], what
    for f in ref.SERIES_FIELDS:
        assert got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), f"{what}: {f}"


def _random_state(words, H, W, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 64, size=(words, H, W), dtype=np.uint64), rng.integers(0, 1 << 64, size=(words, H, W), dtype=np.uint64))


@pytest.fixture(scope="module")
def hard(dev):
    mask, valid_in, conf, hit, valid = ref.hard_stack()
    return dict(mask=mask, valid_in=valid_in, conf=conf, hit=hit, valid=valid, T=mask.shape[0])


# ---- push ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("words,n_dates", [(1, 1), (1, 63), (1, 64), (2, 65), (4, 130), (4, 256)])
def test_push_then_summary(dev, H, W, words, n_dates):
    import insar_unet_ca_amd as iu
    mask, valid_in, conf = ref.random_inputs(H, W, n_dates, 100 + n_dates)
    dm, dv, dc = _t(mask, dev), _t(valid_in, dev), _t(conf, dev)
    st = iu.DetectionStack(H, W, dev, words)
    hit, valid = ref.empty_state(words, H, W)
    t, sizes = 0, [1, 5, 64]
    while t < n_dates:                                            # appended in calls of 1, 5 and 64 dates: 64 from t = 6 crosses a plane
        n = min(sizes[0], n_dates - t)
        sizes = sizes[1:] + sizes[:1]
        sl = slice(t, t + n)
        a = dm[t] if n == 1 else dm[sl]
        assert st.push(a, valid=dv[t] if n == 1 else dv[sl], conf=dc[t] if n == 1 else dc[sl], min_conf=0.5) == t
        hit, valid = ref.push_ref(hit, valid, mask[sl], t, valid_in=valid_in[sl], conf=conf[sl], min_conf=0.5)
        t += n
        assert st.n_dates == t
    _assert_state(st, hit, valid, "push")
    assert np.array_equal(dm.cpu().numpy(), mask) and np.array_equal(dv.cpu().numpy(), valid_in)               # inputs not written
    assert np.array_equal(dc.cpu().numpy().view(np.uint32), conf.view(np.uint32))
    _assert_planes(st.summary(**ref.RULE), ref.summary_ref(hit, valid, 0, n_dates, **ref.RULE), "summary")
    again = st.summary(**ref.RULE)
    first = st.summary(**ref.RULE)
    assert all(again[p].cpu().numpy().tobytes() == first[p].cpu().numpy().tobytes() for p in ref.PLANES)       # identical calls, identical bytes
    t0 = n_dates // 3
    _assert_planes(st.summary(t0, n_dates, min_hits=2), ref.summary_ref(hit, valid, t0, n_dates, min_hits=2), "window")


@pytest.mark.parametrize("H,W", [(37, 203), (200, 264)])
@pytest.mark.parametrize("n,t", [(1, 63), (1, 64), (5, 61), (64, 30), (64, 64), (5, 123), (128, 0)])
def test_overwrite_leaves_every_other_bit(dev, H, W, n, t):
    """Words full of random bits; dates t .. t + n - 1 are overwritten (across planes for most cases). The whole state is
    compared, so the neighbouring bits are checked unchanged."""
    hit, valid = _random_state(2, H, W, 7)
    st = _stack(dev, hit, valid, 128)
    mask, valid_in, conf = ref.random_inputs(H, W, n, 31 + n + t)
    st.push(_t(mask, dev), t, valid=_t(valid_in, dev), conf=_t(conf, dev), min_conf=0.25, classes=(1, 3, 200), ignore=7)
    want = ref.push_ref(hit, valid, mask, t, valid_in=valid_in, conf=conf, min_conf=0.25, classes=(1, 3, 200), ignore=7)
    _assert_state(st, *want, f"overwrite n={n} t={t}")
    assert st.n_dates == 128
    for d in (t - 1, t + n):
        if 0 <= d < 128:
            assert np.array_equal(ref.get_bit(want[0], d), ref.get_bit(hit, d))


@pytest.mark.parametrize("kw", [dict(classes=1), dict(classes=(1, 3, 200)), dict(classes=0), dict(classes=[0, 255], ignore=None),
                                dict(classes=200, ignore=1), dict(classes=(2, 7), ignore=0, min_conf=1.0), dict(min_conf=-1.0)])
@pytest.mark.parametrize("with_valid,with_conf", [(False, False), (True, False), (False, True), (True, True)])
def test_class_sets_ignore_and_optional_inputs(dev, kw, with_valid, with_conf):
    H, W, n = 37, 203, 3
    mask, valid_in, conf = ref.random_inputs(H, W, n, 55)
    hit, valid = _random_state(1, H, W, 8)
    st = _stack(dev, hit, valid, 10)
    st.push(_t(mask, dev), 20, valid=_t(valid_in, dev) if with_valid else None, conf=_t(conf, dev) if with_conf else None, **kw)
    want = ref.push_ref(hit, valid, mask, 20, valid_in=valid_in if with_valid else None, conf=conf if with_conf else None,
                        **{**dict(ignore=255), **kw})
    _assert_state(st, *want, str(kw))
    assert st.n_dates == 23
    assert 0 < int(ref.get_bit(want[0], 21).sum()) < H * W or kw.get("min_conf") == 1.0


def test_conf_equal_to_the_threshold_and_nan(dev):
    import insar_unet_ca_amd as iu
    H, W = 3, 1025
    mask = np.ones((H, W), dtype=np.uint8)
    conf = np.full((H, W), np.float32(0.6), dtype=np.float32)
    conf[0, ::2] = np.nextafter(np.float32(0.6), np.float32(0))
    conf[1, ::3] = np.nan
    conf[2, ::5] = np.inf
    st = iu.DetectionStack(H, W, dev)
    st.push(_t(mask, dev), conf=_t(conf, dev), min_conf=0.6)
    gh, gv = _state(st)
    assert (gv == 1).all()                                         # NaN: valid all the same
    want = np.ones((H, W), dtype=np.uint64)
    want[0, ::2] = 0
    want[1, ::3] = 0
    assert np.array_equal(gh[0], want)


# ---- shift ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,words", [(37, 203, 2), (3, 1025, 4), (200, 264, 1), (1, 1, 3)])
def test_shift_then_summary(dev, H, W, words):
    T = 64 * words
    hit, valid = _random_state(words, H, W, 12)
    for k in (0, 1, 63, 64, 65, T - 1, T, T + 5):
        st = _stack(dev, hit, valid, T)
        st.shift(k)
        want = ref.shift_ref(hit, valid, k)
        _assert_state(st, *want, f"shift {k}")
        assert st.n_dates == max(0, T - k)
        _assert_planes(st.summary(0, T, **ref.RULE), ref.summary_ref(*want, 0, T, **ref.RULE), f"summary after shift {k}")
    st = _stack(dev, hit, valid, T)
    st.shift(3)
    st.shift(2)                                                    # a monitoring job: drop, then append
    mask = np.ones((H, W), dtype=np.uint8)
    st.push(_t(mask, dev))
    want = ref.push_ref(*ref.shift_ref(hit, valid, 5), mask, T - 5)
    _assert_state(st, *want, "shift, shift, push")
    assert st.n_dates == T - 4


# ---- summary -------------------------------------------------------------------------------------------------------------
def test_summary_of_the_hard_stack(dev, hard):
    st = _stack(dev, hard["hit"], hard["valid"], hard["T"])
    T = hard["T"]
    for t0, t1 in ((0, T), (5, 40), (64, 128), (50, 131), (63, 65), (127, 129), (17, 17), (0, 192), (192, 192), (0, 0)):
        _assert_planes(st.summary(t0, t1, **ref.RULE), ref.summary_ref(hard["hit"], hard["valid"], t0, t1, **ref.RULE), f"{t0}..{t1}")
    empty = st.summary(9, 9, min_hits=0, min_run=0, min_valid=0)
    assert (empty["persistent"] == 1).all() and (empty["known"] == 1).all() and (empty["run_start"] == -1).all()
    assert (st.summary(9, 9)["persistent"] == 0).all()
    full = ref.summary_ref(hard["hit"], hard["valid"], 0, T, **ref.RULE)
    f = lambda p: full[p].reshape(-1)
    assert (f("longest_run")[:150] == 5).all() and (f("run_start")[:150] == 10).all()                # bridged: 10, 11, (12), 13, 14, 15
    assert (f("longest_run")[150:180] == 3).all() and (f("run_start")[150:180] == 20).all()          # the earlier of two
    assert (f("run_start")[200:220] == 60).all() and (f("longest_run")[200:220] == 9).all()
    assert (f("run_start")[220:240] == 125).all() and (f("longest_run")[220:240] == 6).all()


def test_each_rule_parameter_at_and_past_its_boundary(dev, hard):
    st = _stack(dev, hard["hit"], hard["valid"], hard["T"])
    T = hard["T"]
    s = ref.summary_ref(hard["hit"], hard["valid"], 0, T)
    pix = 5                                                       # a planted pixel: 5 hits in one run of 5, 130 valid dates
    a, b, c = (int(s[k].reshape(-1)[pix]) for k in ("n_hit", "longest_run", "n_valid"))
    assert (a, b, c) == (5, 5, T - 1)
    cases = [(dict(min_hits=a), 1), (dict(min_hits=a + 1), 0), (dict(min_run=b), 1), (dict(min_run=b + 1), 0), (dict(min_valid=c), 1),
             (dict(min_valid=c + 1), 0), (dict(min_fraction=(a, c)), 1), (dict(min_fraction=(a + 1, c)), 0), (dict(min_fraction=(1, 26)), 1),
             (dict(min_fraction=(1, 25)), 0), (dict(min_run=0, min_hits=0, min_valid=0), 1), (dict(min_fraction=(1, 1)), 0),
             (dict(min_hits=32767), 0), (dict(min_fraction=(1, (1 << 31) - 1)), 1)]
    for rule, want_pix in cases:
        for want in (("persistent",), ("persistent", "known", "longest_run")):                       # without and with the run scan
            got = st.summary(0, T, want=want, **rule)
            w = ref.summary_ref(hard["hit"], hard["valid"], 0, T, **rule)
            _assert_planes(got, w, str(rule), planes=want)
            assert int(w["persistent"].reshape(-1)[pix]) == want_pix, rule
    k = st.summary(0, T, want=("known",), min_valid=c + 1)["known"].cpu().numpy().reshape(-1)
    assert k[pix] == 0 and k[190] == 1


def test_want_subsets_allocate_only_what_is_asked(dev, hard):
    st = _stack(dev, hard["hit"], hard["valid"], hard["T"])
    want_all = ref.summary_ref(hard["hit"], hard["valid"], 3, 120, **ref.RULE)
    for p in ref.PLANES:
        got = st.summary(3, 120, want=(p,), **ref.RULE)
        assert list(got) == [p]
        _assert_planes(got, want_all, p, planes=(p,))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    got = st.summary(3, 120, want=("persistent", "first_hit"), **ref.RULE)
    assert torch.cuda.memory_allocated() - base <= 2 * (512 + 3 * 200 * 264)                         # one uint8 and one int16 plane
    _assert_planes(got, want_all, "pair", planes=("persistent", "first_hit"))
    _assert_planes(st.summary(3, 120, want="n_hit"), want_all, "str", planes=("n_hit",))


# ---- series --------------------------------------------------------------------------------------------------------------
def _series(dev, hard, labels, what, **kw):
    import insar_unet_ca_amd as iu
    st = _stack(dev, hard["hit"], hard["valid"], hard["T"])
    dl = _t(labels.astype(np.int32), dev)
    got = iu.site_series(st, dl, **kw)
    want = ref.series_ref(hard["hit"], hard["valid"], labels, **{**dict(t1=hard["T"]), **kw})
    _assert_series(got, want, what)
    assert np.array_equal(dl.cpu().numpy(), labels)
    _assert_state(st, hard["hit"], hard["valid"], what)
    return got, want


def test_series_random_patches(dev, hard):
    lab = ref.series_labels(200, 264, 21, max_regions=40)
    got, want = _series(dev, hard, lab, "patches", max_regions=40)
    assert want["out_of_range"] > 20 and (want["area"] > 0).sum() > 20 and want["hits"].sum() > 1000
    _series(dev, hard, lab, "patches, count", max_regions=64, count=20)
    _series(dev, hard, lab, "patches, small table", max_regions=5)
    _series(dev, hard, lab, "patches, count 0", max_regions=40, count=0)
    for t0, t1 in ((50, 131), (0, 64), (63, 65), (64, 128), (100, 100), (0, 192)):
        _series(dev, hard, lab, f"patches {t0}..{t1}", max_regions=40, t0=t0, t1=t1, active_fraction=(1, 3))
    _series(dev, hard, lab, "patches, default table", count=45)


def test_series_one_region_covering_the_map(dev, hard):
    got, want = _series(dev, hard, np.ones((200, 264), dtype=np.int32), "one region", max_regions=1)
    assert got["area"][0] == 200 * 264 and got["valids"][0].max() > 40000
    _series(dev, hard, np.full((200, 264), 3, dtype=np.int32), "one region, id 3 of 4", max_regions=4, t0=60, t1=70)
    halves = np.ones((200, 264), dtype=np.int32)
    halves[100:] = 2                                              # the hot label changes once per work-group at most
    _series(dev, hard, halves, "two halves", max_regions=2)


def test_series_ten_thousand_single_pixel_regions(dev, hard):
    lab = np.zeros(200 * 264, dtype=np.int32)
    lab[:10000] = np.random.default_rng(3).permutation(10000) + 1
    got, want = _series(dev, hard, lab.reshape(200, 264), "single pixels", max_regions=10000)
    assert (got["area"] == 1).all()
    stripes = (1 + (np.arange(264) // 5)).astype(np.int32)[None, :].repeat(200, axis=0)
    _series(dev, hard, stripes, "stripes of 5", max_regions=int(stripes.max()))
    alt = (1 + (np.arange(200 * 264) % 3)).reshape(200, 264).astype(np.int32)
    _series(dev, hard, alt, "period 3", max_regions=3)


@pytest.mark.parametrize("H,W", [(37, 203), (1, 1), (3, 1025)])
def test_series_on_ragged_maps_with_a_reused_scratch(dev, H, W):
    import insar_unet_ca_amd as iu
    hit, valid = _random_state(2, H, W, 5)
    st = _stack(dev, hit, valid, 128)
    rng = np.random.default_rng(6)
    lab = rng.integers(-1, 9, size=(H, W)).astype(np.int32)
    sc = iu.StackScratch(dev, 6, 100)
    sc.table.fill_(0xAB)                                           # whatever the table held is cleared
    a = iu.site_series(st, _t(lab, dev), max_regions=6, t0=20, t1=120, scratch=sc)
    _assert_series(a, ref.series_ref(hit, valid, lab, max_regions=6, t0=20, t1=120), "scratch")
    raw = sc.table.cpu().numpy().tobytes()
    b = iu.site_series(st, _t(lab, dev), max_regions=6, t0=20, t1=120, scratch=sc)
    assert sc.table.cpu().numpy().tobytes() == raw                 # identical calls, identical bytes
    _assert_series(b, a, "again")


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _assert_follow(out, hit, valid, t0, t1, rule, active_fraction, what):
    planes = ref.summary_ref(hit, valid, t0, t1, **rule)
    _assert_planes(out["summary"], planes, what)
    labels = out["labels"].cpu().numpy()
    assert np.array_equal(labels > 0, planes["persistent"] == 1), what                               # min_area = 1: every persistent pixel is in a site
    assert out["count"] == int(labels.max()) == len(out["regions"]["id"])
    want = ref.series_ref(hit, valid, labels, max_regions=65536, count=out["count"], t0=t0, t1=t1, active_fraction=active_fraction)
    _assert_series(out, want, what)
    assert np.array_equal(out["area"], out["regions"]["area"]), what                                 # rows aligned with regions["id"]


def test_follow_sites(dev, hard):
    import insar_unet_ca_amd as iu
    st = _stack(dev, hard["hit"], hard["valid"], hard["T"])
    out = iu.follow_sites(st, **ref.RULE)
    _assert_follow(out, hard["hit"], hard["valid"], 0, hard["T"], ref.RULE, (1, 2), "follow")
    assert out["count"] > 10 and (out["onset"] >= 0).sum() > 5 and (out["t0"], out["t1"]) == (0, hard["T"])
    rule = dict(min_hits=4, min_run=3)
    out = iu.follow_sites(st, t0=40, t1=131, active_fraction=(1, 3), want=("n_hit",), connectivity=4, **rule)
    assert set(out["summary"]) == {"n_hit", "persistent"}
    want = ref.summary_ref(hard["hit"], hard["valid"], 40, 131, **rule)
    _assert_planes(out["summary"], want, "follow, window", planes=("n_hit", "persistent"))
    labels = out["labels"].cpu().numpy()
    assert np.array_equal(labels > 0, want["persistent"] == 1)
    _assert_series(out, ref.series_ref(hard["hit"], hard["valid"], labels, max_regions=65536, count=out["count"], t0=40, t1=131,
                                       active_fraction=(1, 3)), "follow, window")
    big = iu.follow_sites(st, min_area=30, **ref.RULE)
    assert 0 < big["count"] < iu.follow_sites(st, **ref.RULE)["count"] and (big["area"] >= 30).all()


def test_detect_stack_end_to_end(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    rng = np.random.default_rng(4)
    base = rng.standard_normal((64, 80)).astype(np.float32)
    scenes = [base + 0.3 * rng.standard_normal((64, 80)).astype(np.float32) for _ in range(3)]
    pred = iu.ScenePredictor(net, tile=32, overlap=8, batch=4, num_classes=2)
    p = pred.predict(scenes[0], return_prob=True)["prob"]
    with torch.no_grad():                                          # an untrained net: split the class map about evenly
        net.outc.bias[1] += torch.log(p[0] / p[1]).median()
    valids = [None, (rng.random((64, 80)) < 0.8).astype(np.uint8), None]
    mc = float(np.median(pred.predict(scenes[1])["conf"].cpu().numpy()))
    rule = dict(min_hits=2, min_run=2, min_valid=2)
    out = pred.detect_stack(scenes, valids=valids, min_conf=mc, min_area=2, **rule)
    st = out["stack"]
    assert st.n_dates == 3 and st.words == 1 and tuple(st.hit.shape) == (1, 64, 80)
    hit, valid = ref.empty_state(1, 64, 80)
    for i, s in enumerate(scenes):                                # the restatement on the predictor's own masks
        o = pred.predict(s)
        hit, valid = ref.push_ref(hit, valid, o["mask"].cpu().numpy(), i, valid_in=valids[i], conf=o["conf"].cpu().numpy(), min_conf=mc)
    _assert_state(st, hit, valid, "detect_stack")
    planes = ref.summary_ref(hit, valid, 0, 3, **rule)
    _assert_planes(out["summary"], planes, "detect_stack")
    assert 0 < int(planes["persistent"].sum()) < 64 * 80
    labels = out["labels"].cpu().numpy()
    assert ((labels > 0) <= (planes["persistent"] == 1)).all() and out["count"] > 0                  # min_area = 2 drops single pixels
    _assert_series(out, ref.series_ref(hit, valid, labels, max_regions=65536, count=out["count"], t0=0, t1=3), "detect_stack")
    again = pred.detect_stack(scenes, valids=valids, min_conf=mc, min_area=2, **rule)
    assert torch.equal(again["stack"].hit, st.hit) and torch.equal(again["labels"], out["labels"])
    assert all(np.asarray(again[f]).tobytes() == np.asarray(out[f]).tobytes() for f in ref.SERIES_FIELDS)
    wide = pred.detect_stack(scenes, words=2, **rule)
    assert tuple(wide["stack"].hit.shape) == (2, 64, 80) and wide["hits"].shape[1] == 3
