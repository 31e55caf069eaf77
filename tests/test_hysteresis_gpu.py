"""GPU: hysteresis thresholds (insar_unet_ca_amd/hysteresis.py on csrc/hysteresis.hip and the insar_regions_* phases) against the
numpy restatement of tests/hysteresis_ref.py (pinned on hand-built cases in tests/test_hysteresis_host.py, which also asserts
that the maps used here hold a kept region, a component dropped for lack of a seed and a region seeded only from another
labelling tile) and against `label_regions`.

Every comparison is exact: labels, mask, conf, count, candidates and every field of the table. Shapes: 1 x 1, 1 x 7, 5 x 3
(smaller than a quad row), 33 x 65 and 97 x 130 (odd widths take the guarded path and cross the 32 x 64 labelling tiles; with
three planes the plane offsets lose the 16-byte alignment), 64 x 128 (the vector path, several work-groups)."""
import functools

import numpy as np
import pytest
import torch

from insar_unet_ca_amd._lib import InsarError
from tests import hysteresis_ref as ref

pytestmark = pytest.mark.gpu
LOW, HIGH = ref.LOW, ref.HIGH
FIELDS = ("id", "cls", "area", "y0", "x0", "y1", "x1", "cy", "cx", "mean_conf", "n_seed", "peak", "peak_y", "peak_x")
DTYPES = {"id": np.int32, "cls": np.int32, "area": np.int64, "cy": np.float64, "mean_conf": np.float64, "n_seed": np.int64,
          "peak": np.float32, "peak_y": np.int32, "peak_x": np.int32}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _scores(H, W, K):
    return ref.blob_scores(H, W, H * 1000 + W, K)


@functools.lru_cache(maxsize=None)
def _valid(H, W):
    return ref.valid_map(H, W, H * 1000 + W)


@functools.lru_cache(maxsize=None)
def _want(H, W, K, conn, with_valid, low=LOW, high=HIGH, min_area=1, min_seeds=1):
    return ref.hysteresis(_scores(H, W, K), low, high, valid=_valid(H, W) if with_valid else None, connectivity=conn,
                          min_area=min_area, min_seeds=min_seeds)


def _same(out, want, what=""):
    print(f"{what}: {out['count']} regions of {out['candidates']} candidates, restatement {want['count']} of {want['candidates']}")
    assert (out["count"], out["candidates"]) == (want["count"], want["candidates"]), what
    assert out["labels"].dtype == torch.int32 and out["mask"].dtype == torch.uint8 and out["conf"].dtype == torch.float32
    assert np.array_equal(out["labels"].cpu().numpy(), want["labels"]), f"{what}: labels"
    assert np.array_equal(out["mask"].cpu().numpy(), want["mask"]), f"{what}: mask"
    assert out["conf"].cpu().numpy().tobytes() == want["conf"].tobytes(), f"{what}: conf"
    assert set(out["regions"]) == set(FIELDS), what
    for f in FIELDS:
        got, exp = out["regions"][f], want["regions"][f]
        assert got.shape == (want["count"],) and got.dtype == DTYPES.get(f, got.dtype), f"{what}: {f} {got.dtype} {got.shape}"
        assert got.tobytes() == exp.astype(got.dtype).tobytes(), f"{what}: {f}"


def _same_bits(a, b):
    for k in ("labels", "mask", "conf"):
        assert torch.equal(a[k], b[k]), k
    assert (a["count"], a["candidates"]) == (b["count"], b["candidates"])
    for f in FIELDS:
        assert a["regions"][f].tobytes() == b["regions"][f].tobytes(), f


# ---- against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_valid", [False, True], ids=["all_valid", "valid"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("H,W", ref.SHAPES)
def test_blob_maps(dev, H, W, conn, K, with_valid):
    import insar_unet_ca_amd as iu
    out = iu.hysteresis_regions(_t(_scores(H, W, K), dev), LOW, HIGH, valid=_t(_valid(H, W), dev) if with_valid else None,
                                connectivity=conn)
    _same(out, _want(H, W, K, conn, with_valid), f"{H} x {W}, K {K}, connectivity {conn}, valid {with_valid}")


def test_per_class_thresholds_class_subsets_and_min_area(dev):
    import insar_unet_ca_amd as iu
    s = _scores(97, 130, 3)
    t = _t(s, dev)
    for low, high, classes, min_area in (({1: 0.25, 2: 0.125}, {1: 0.75, 2: 0.5}, None, 1), ([9, 0.5, 0.25], [9, 0.5, 1.0], None, 3),
                                         (0.25, 0.75, [2], 1), ({1: 0.375}, {1: 0.625}, (1,), 6), (-1.0, 0.75, None, 2)):
        out = iu.hysteresis_regions(t, low, high, classes=classes, min_area=min_area, connectivity=4)
        want = ref.hysteresis(s, low, high, classes=classes, min_area=min_area, connectivity=4)
        _same(out, want, f"low {low}, high {high}, classes {classes}, min_area {min_area}")
        assert want["count"] > 0
    # p(background) above every class: the class is a candidate all the same
    two = np.stack([np.full((5, 3), 0.7, np.float32), np.full((5, 3), 0.3, np.float32)])
    out = iu.hysteresis_regions(_t(two, dev), 0.2, 0.3)
    assert out["count"] == 1 and out["regions"]["area"].tolist() == [15] and bool((out["mask"] == 1).all())


def test_negative_scores_keep_their_exact_peak(dev):
    import insar_unet_ca_amd as iu
    s = np.full((5, 3), -0.5, dtype=np.float32)
    s[3, 1], s[4, 2], s[0, 0] = -0.25, -0.25, np.nan
    out = iu.hysteresis_regions(_t(s, dev), -1.0, -0.3)
    _same(out, ref.hysteresis(s, -1.0, -0.3), "negative scores")
    r = out["regions"]
    assert (r["peak"].tolist(), r["peak_y"].tolist(), r["peak_x"].tolist(), r["n_seed"].tolist()) == ([-0.25], [3], [1], [2])
    z = np.array([[-0.0, 0.0, -0.0, 0.0]], dtype=np.float32)      # -0.0 orders below 0.0: the first +0.0 is the peak
    out = iu.hysteresis_regions(_t(z, dev), -1.0, 0.0)
    _same(out, ref.hysteresis(z, -1.0, 0.0), "signed zeros")
    assert out["regions"]["peak_x"].tolist() == [1] and out["regions"]["n_seed"].tolist() == [4]


def test_isolated_seeds_fill_three_passes_of_keep(dev):
    """2500 one-pixel sites: `keep` scans 1024 records per pass, so it runs three passes and carries the kept count from one to
    the next and into the header. The expected labels are 1..2500 in row-major order; the capacity is exact."""
    import insar_unet_ca_amd as iu
    s = np.zeros((100, 100), dtype=np.float32)
    s[1::2, 1::2] = 1.0
    out = iu.hysteresis_regions(_t(s, dev), 0.25, 0.75, connectivity=4, min_seeds=1, max_regions=2500)
    _same(out, ref.hysteresis(s, 0.25, 0.75, connectivity=4, min_seeds=1), "isolated seeds")
    labels = np.zeros((100, 100), dtype=np.int32)
    labels[1::2, 1::2] = np.arange(1, 2501, dtype=np.int32).reshape(50, 50)
    assert out["count"] == out["candidates"] == 2500 and np.array_equal(out["labels"].cpu().numpy(), labels)
    r = out["regions"]
    assert np.array_equal(r["id"], np.arange(1, 2501)) and (r["area"] == 1).all() and (r["n_seed"] == 1).all()
    assert np.array_equal(r["peak_y"], np.nonzero(labels)[0]) and np.array_equal(r["peak_x"], np.nonzero(labels)[1])


# ---- the identities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("H,W,K", [(33, 65, 1), (64, 128, 3), (97, 130, 2)])
def test_low_equal_high_is_label_regions(dev, H, W, K, conn):
    import insar_unet_ca_amd as iu
    for t, min_area in ((0.25, 1), (0.5, 4)):
        out = iu.hysteresis_regions(_t(_scores(H, W, K), dev), t, t, connectivity=conn, min_area=min_area)
        cand, conf, _ = ref.candidates(_scores(H, W, K), t, t)
        reg = iu.label_regions(_t(cand, dev), _t(conf, dev), connectivity=conn, min_area=min_area)
        assert out["conf"].cpu().numpy().tobytes() == conf.tobytes()
        assert out["count"] == out["candidates"] == reg["count"] > 0
        assert torch.equal(out["labels"], reg["labels"]) and torch.equal(out["mask"], reg["mask"])
        assert set(reg["regions"]) < set(out["regions"])
        for f, v in reg["regions"].items():
            assert out["regions"][f].dtype == v.dtype and out["regions"][f].tobytes() == v.tobytes(), f
        assert np.array_equal(out["regions"]["n_seed"], out["regions"]["area"])


@pytest.mark.parametrize("H,W,K", [(33, 65, 2), (97, 130, 3)])
def test_raising_high_only_removes_regions(dev, H, W, K):
    import insar_unet_ca_amd as iu
    t = _t(_scores(H, W, K), dev)
    prev, counts = None, []
    for high in (0.25, 0.5, 0.75, 1.0):
        out = iu.hysteresis_regions(t, 0.25, high)
        lab = out["labels"].cpu().numpy().ravel()
        sets = {frozenset(np.flatnonzero(lab == k).tolist()) for k in range(1, out["count"] + 1)}
        assert len(sets) == out["count"] and (prev is None or sets <= prev)
        prev = sets
        counts.append(out["count"])
    print(f"{H} x {W}, K {K}: kept {counts} as high rises")
    assert counts[0] > counts[2] > 0 and counts == sorted(counts, reverse=True)


# ---- min_seeds, max_regions, scratch, launches ---------------------------------------------------------------------------
def test_min_seeds(dev):
    import insar_unet_ca_amd as iu
    t = _t(_scores(97, 130, 2), dev)
    most = int(_want(97, 130, 2, 8, False)["regions"]["n_seed"].max())
    kept = []
    for min_seeds in (1, 2, most, most + 1):
        out = iu.hysteresis_regions(t, LOW, HIGH, min_seeds=min_seeds)
        _same(out, _want(97, 130, 2, 8, False, min_seeds=min_seeds), f"min_seeds {min_seeds}")
        kept.append(out["count"])
    assert kept[0] > kept[1] >= kept[2] >= 1 and kept[3] == 0     # the streak has one seed; above every region's seeds: none, no error
    assert not bool(out["labels"].any()) and not bool(out["mask"].any()) and out["candidates"] > 0


def test_max_regions_overflow_raises(dev):
    import insar_unet_ca_amd as iu
    t = _t(_scores(64, 128, 3), dev)
    want = _want(64, 128, 3, 8, False)
    n = want["candidates"]
    assert n > want["count"] > 1
    with pytest.raises(InsarError, match=f"hysteresis_regions: {n} regions .* exceed max_regions={n - 1}"):
        iu.hysteresis_regions(t, LOW, HIGH, max_regions=n - 1)                 # the cap counts the components BEFORE the seed rule
    with pytest.raises(InsarError, match="max_regions=1"):
        iu.hysteresis_regions(t, LOW, HIGH, max_regions=1)
    _same(iu.hysteresis_regions(t, LOW, HIGH, max_regions=n), want, "exactly max_regions")


def test_reused_scratch_and_repeated_calls_give_the_same_bits(dev):
    import insar_unet_ca_amd as iu
    t, other = _t(_scores(97, 130, 3), dev), _t(ref.blob_scores(97, 130, 77, 3), dev)
    v = _t(_valid(97, 130), dev)
    scratch = iu.HysteresisScratch(97, 130, dev, max_regions=500)
    kw = dict(connectivity=4, max_regions=500)
    fresh = iu.hysteresis_regions(t, LOW, HIGH, valid=v, **kw)
    again = iu.hysteresis_regions(t, LOW, HIGH, valid=v, **kw)
    a = iu.hysteresis_regions(t, LOW, HIGH, valid=v, scratch=scratch, **kw)
    iu.hysteresis_regions(other, 0.25, 0.5, min_seeds=3, scratch=scratch, max_regions=500)
    b = iu.hysteresis_regions(t, LOW, HIGH, valid=v, scratch=scratch, **kw)
    _same(fresh, _want(97, 130, 3, 4, True), "fresh scratch")
    for x in (again, a, b):
        _same_bits(fresh, x)
    with pytest.raises(InsarError, match="scratch of"):
        iu.hysteresis_regions(t, LOW, HIGH, scratch=scratch)
    with pytest.raises(InsarError, match="scratch of"):
        iu.hysteresis_regions(_t(_scores(64, 128, 2), dev), LOW, HIGH, scratch=scratch, max_regions=500)


def test_launch_count(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd import hysteresis as hy
    per_call = {"insar_hyst_classify": 1, "insar_regions_tiles": 1, "insar_regions_merge": 1, "insar_regions_flatten": 1,
                "insar_regions_number": 3, "insar_regions_relabel": 1, "insar_hyst_seeds": 2, "insar_hyst_keep": 1, "insar_hyst_apply": 1}
    for H, W, K in ((1, 1, 1), (97, 130, 3)):
        t = _t(_scores(H, W, K), dev)
        tape = []
        _lib._TAPE = tape
        try:
            iu.hysteresis_regions(t, LOW, HIGH)
        finally:
            _lib._TAPE = None
        names = [n for _, _, n in tape]                          # the host-only size queries launch nothing
        assert sorted(set(names) - {"insar_hyst_scratch_bytes", "insar_regions_scratch_bytes"}) == sorted(per_call), names
        assert sum(per_call.get(n, 0) for n in names) == hy.LAUNCHES == 12, names


# ---- the scene pipeline ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predictor(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    scene = np.random.default_rng(4).standard_normal((96, 96)).astype(np.float32)
    pred = iu.ScenePredictor(net, tile=32, overlap=8, batch=4, num_classes=2)
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():                                         # split the class map about evenly (tests/test_outlines_gpu.py)
        net.outc.bias[1] += torch.log(p[0] / p[1]).median()
    p1 = pred.predict(scene, return_prob=True)["prob"][1].cpu().numpy()
    low, high = float(np.quantile(p1, 0.35)), float(np.quantile(p1, 0.9))          # from the input of the tool, not from its output
    return pred, scene, low, high


def _equal(x, y):
    if isinstance(x, torch.Tensor):
        return torch.equal(x, y)
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_equal(x[k], y[k]) for k in x)
    if isinstance(x, np.ndarray):
        return x.tobytes() == y.tobytes()
    return x == y


def test_detect_grows_sites_from_seeds(dev, predictor):
    import insar_unet_ca_amd as iu
    pred, scene, low, high = predictor
    kw = dict(connectivity=4, min_area=2)
    plain = pred.predict(scene, return_prob=True)
    det = pred.detect(scene, hysteresis=(low, high), **kw)
    by_hand = iu.hysteresis_regions(plain["prob"], low, high, **kw)
    want = ref.hysteresis(plain["prob"].cpu().numpy(), low, high, **kw)
    _same(by_hand, want, "detect, by hand")
    assert want["count"] > 1 and want["unseeded"] > 0
    assert set(det) == {"mask", "conf", "labels", "regions", "count", "mask_clean", "conf_hysteresis", "hysteresis_candidates"}
    assert torch.equal(det["mask"], plain["mask"]) and torch.equal(det["conf"], plain["conf"])
    assert torch.equal(det["labels"], by_hand["labels"]) and torch.equal(det["mask_clean"], by_hand["mask"])
    assert torch.equal(det["conf_hysteresis"], by_hand["conf"]) and det["count"] == by_hand["count"]
    assert det["hysteresis_candidates"] == by_hand["candidates"] and _equal(det["regions"], by_hand["regions"])
    # sites reach below the arg-max boundary: pixels that the arg-max map calls background are labelled
    assert bool(((det["labels"] > 0) & (plain["mask"] == 0)).any())
    with_prob = pred.detect(scene, return_prob=True, hysteresis={"low": low, "high": high, "min_seeds": 1}, **kw)
    assert set(with_prob) == set(det) | {"prob"} and torch.equal(with_prob["prob"], plain["prob"])
    assert torch.equal(with_prob["labels"], det["labels"])
    two = pred.detect(scene, hysteresis={"low": low, "high": high, "min_seeds": 2, "connectivity": 8}, **kw)
    assert _equal(two["regions"], iu.hysteresis_regions(plain["prob"], low, high, min_seeds=2, connectivity=8, min_area=2)["regions"])
    # what runs on the regions runs on these
    full = pred.detect(scene, hysteresis=(low, high), outlines=True, skeletons=True, measure={"p": plain["prob"][1]}, split=True, **kw)
    assert {"outlines", "skeleton", "stats", "split_rounds"} <= set(full) and len(full["regions"]["perimeter"]) == full["count"]
    one = iu.detect_scene(pred.model, scene, hysteresis=(low, high), tile=32, overlap=8, batch=4, num_classes=2, **kw)
    assert torch.equal(one["labels"], det["labels"])
    for bad, msg in ((dict(sieve={1: 8}), "sieve next to hysteresis"), (dict(min_conf=0.6), "min_conf next to hysteresis")):
        with pytest.raises(InsarError, match=msg):
            pred.detect(scene, hysteresis=(low, high), **bad)
    with pytest.raises(InsarError, match=r"low\[1\]=.* > high\[1\]"):
        pred.detect(scene, hysteresis=(high, low))
    print(f"detect: {det['count']} sites of {det['hysteresis_candidates']} candidates at low {low:.3f}, high {high:.3f}")


def test_detect_with_valid_labels_no_invalid_pixel(dev, predictor):
    pred, scene, low, high = predictor
    valid = np.ones((96, 96), dtype=np.uint8)
    valid[:, 40:56] = 0
    valid[70:, :] = 0
    det = pred.detect(scene, hysteresis=(0.0, high), valid=valid, min_area=1)
    off = torch.from_numpy(valid == 0).to(det["labels"].device)
    assert torch.equal(det["valid"].cpu(), torch.from_numpy(valid))
    assert not det["labels"][off].any() and not det["mask_clean"][off].any() and not det["conf_hysteresis"][off].any()
    assert bool((det["conf_hysteresis"][~off] > 0).all())         # low = 0: every valid pixel is a candidate
    assert det["count"] >= 1 and int(det["regions"]["area"].sum()) == int((det["labels"] > 0).sum()) > 0
    free = pred.detect(scene, hysteresis=(0.0, high), min_area=1)  # without `valid` the same thresholds label the whole scene
    assert free["count"] == 1 and bool((free["labels"] == 1).all()) and "valid" not in free


def test_detect_without_hysteresis_is_unchanged(dev, predictor):
    import insar_unet_ca_amd as iu
    pred, scene, _, _ = predictor
    kw = dict(connectivity=8, min_area=2, min_conf=0.55)
    a, b = pred.detect(scene, **kw), pred.detect(scene, hysteresis=None, **kw)
    by_hand = pred.predict(scene)
    reg = iu.label_regions(by_hand["mask"], by_hand["conf"], **kw)
    assert a.keys() == b.keys() == {"mask", "conf", "labels", "regions", "count", "mask_clean"}
    assert _equal(a, b)
    assert torch.equal(a["labels"], reg["labels"]) and torch.equal(a["mask_clean"], reg["mask"]) and _equal(a["regions"], reg["regions"])


def test_evaluate_scores_the_hysteresis_labels(dev, predictor):
    import insar_unet_ca_amd as iu
    pred, scene, low, high = predictor
    gt = (np.nan_to_num(ref.blob_scores(96, 96, 9, 1)) >= 0.5).astype(np.uint8)
    gt[:4, :] = 255
    kw = dict(connectivity=8, min_area=2)
    out = pred.evaluate(scene, gt, hysteresis=(low, high), **kw)
    det = pred.detect(scene, hysteresis=(low, high), **kw)
    plain = pred.evaluate(scene, gt, **kw)
    assert torch.equal(out["labels"], det["labels"]) and out["count"] == det["count"] and _equal(out["regions"], det["regions"])
    assert out["hysteresis_candidates"] == det["hysteresis_candidates"]
    assert out["gt_count"] == plain["gt_count"] > 0 and torch.equal(out["gt_labels"], plain["gt_labels"])
    assert len(out["score"]["pred_match"]) == out["count"] and len(out["score"]["gt_match"]) == out["gt_count"]
    one = iu.evaluate_scene(pred.model, scene, gt, hysteresis=(low, high), tile=32, overlap=8, batch=4, num_classes=2, **kw)
    assert torch.equal(one["labels"], out["labels"])
