"""GPU: the region adjacency table and the sieve (insar_unet_ca_amd/sieve.py on csrc/sieve.hip) against the numpy restatement of
tests/sieve_ref.py (pinned on the prototype's findings in tests/test_sieve_host.py) and against the existing tools.

Every comparison is exact: the pairs and their edge counts, the cleaned map, the roots, absorbed, changed_pixels, rounds and
converged. Shapes: 1 x 1, 1 x 7, 5 x 3 (smaller than a quad row), 33 x 65 and 97 x 130 (odd widths take the guarded path and cross
the 32 x 64 labelling tiles), 64 x 128 (the vector path, several work-groups)."""
import functools

import numpy as np
import pytest
import torch

from insar_unet_ca_amd._lib import InsarError
from tests import sieve_ref as ref

pytestmark = pytest.mark.gpu
T2 = {0: 9, 1: 14}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _map(H, W):
    return ref.blob_speckle(H, W, seed=H * 1000 + W)


@functools.lru_cache(maxsize=None)
def _labels(H, W, conn):
    return ref.label_all(_map(H, W), conn)[0]


@functools.lru_cache(maxsize=None)
def _sieved(H, W, conn):
    return ref.sieve(_map(H, W), T2, connectivity=conn)


def _same_pairs(adj, want, what=""):
    print(f"{what}: {adj['count']} pairs, restatement {want['count']}")
    assert adj["count"] == want["count"], what
    assert adj["a"].dtype == np.int32 and adj["b"].dtype == np.int32 and adj["edges"].dtype == np.int64
    for f in ("a", "b", "edges"):
        assert np.array_equal(adj[f], want[f]), f"{what}: {f}"


def _same_sieve(out, want, m, what=""):
    got = (out["regions_in"], out["absorbed"], out["changed_pixels"], out["rounds"], out["converged"])
    exp = (want["regions_in"], want["absorbed"], want["changed_pixels"], want["rounds"], want["converged"])
    print(f"{what}: (regions, absorbed, changed, rounds, converged) = {got}, restatement {exp}")
    assert got == exp, what
    assert out["mask"].dtype == torch.uint8 and out["labels_in"].dtype == torch.int32 and out["root"].dtype == np.int32
    assert np.array_equal(out["labels_in"].cpu().numpy(), want["labels_in"]), f"{what}: labels_in"
    assert np.array_equal(out["root"], want["root"]), f"{what}: root"
    mask = out["mask"].cpu().numpy()
    assert np.array_equal(mask, want["mask"]), f"{what}: {(mask != want['mask']).sum()} pixels differ"
    if "changed" in out:
        assert np.array_equal(out["changed"].cpu().numpy(), (mask != m).astype(np.uint8)), f"{what}: changed"


# ---- region_adjacency --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("H,W", ref.SHAPES)
def test_adjacency_of_all_class_regions(dev, H, W, conn):
    import insar_unet_ca_amd as iu
    labels = _labels(H, W, conn)
    _same_pairs(iu.region_adjacency(_t(labels, dev)), ref.adjacency(labels), f"{H} x {W}, connectivity {conn}")


def test_adjacency_of_a_checkerboard_and_of_one_region(dev):
    import insar_unet_ca_amd as iu
    H, W = 64, 128
    board = np.arange(1, H * W + 1, dtype=np.int32).reshape(H, W)              # every pixel its own region: the most pairs per pixel
    adj = iu.region_adjacency(_t(board, dev), max_pairs=1 << 14)
    _same_pairs(adj, ref.adjacency(board), "checkerboard")
    assert adj["count"] == H * (W - 1) + (H - 1) * W and (adj["edges"] == 1).all()
    for shape in ((64, 128), (33, 65)):
        one = iu.region_adjacency(_t(np.full(shape, 3, dtype=np.int32), dev))
        assert one["count"] == 0 and one["a"].shape == (0,) and one["edges"].shape == (0,)
    two = np.ones((40, 64), dtype=np.int32)                        # one long border: folded per thread and per wave run
    two[17:, :] = 2
    adj = iu.region_adjacency(_t(two, dev))
    assert (adj["a"].tolist(), adj["b"].tolist(), adj["edges"].tolist()) == ([1], [2], [64])


def test_adjacency_of_non_contiguous_ids_and_background(dev):
    import insar_unet_ca_amd as iu
    labels = _labels(97, 130, 8).astype(np.int64)
    split_like = np.where(labels % 5 == 0, 0, labels * 7919 + 100000).astype(np.int32)      # sparse ids, some <= 0
    split_like[labels % 11 == 0] = -4
    for m in (split_like, np.ascontiguousarray(split_like[:64, :128])):
        _same_pairs(iu.region_adjacency(_t(m, dev)), ref.adjacency(np.where(m > 0, m, 0)), f"sparse ids {m.shape}")
    big = np.full((8, 16), (1 << 31) - 1, dtype=np.int32)
    big[:, 8:] = (1 << 31) - 2
    adj = iu.region_adjacency(_t(big, dev))
    assert (adj["a"].tolist(), adj["b"].tolist(), adj["edges"].tolist()) == ([(1 << 31) - 2], [(1 << 31) - 1], [8])


def test_adjacency_max_pairs_too_small_raises(dev):
    import insar_unet_ca_amd as iu
    labels = _t(_labels(64, 128, 4), dev)
    n = ref.adjacency(_labels(64, 128, 4))["count"]
    assert n > 64
    with pytest.raises(InsarError, match="max_pairs=8"):
        iu.region_adjacency(labels, max_pairs=8)
    with pytest.raises(InsarError, match=f"max_pairs={n - 1}"):
        iu.region_adjacency(labels, max_pairs=n - 1)
    assert iu.region_adjacency(labels, max_pairs=n)["count"] == n


# ---- sieve_regions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("H,W", ref.SHAPES)
def test_blob_and_speckle_maps(dev, H, W, conn):
    import insar_unet_ca_amd as iu
    m = _map(H, W)
    out = iu.sieve_regions(_t(m, dev), min_area=T2, connectivity=conn, return_changed=True)
    _same_sieve(out, _sieved(H, W, conn), m, f"{H} x {W}, connectivity {conn}")


@pytest.mark.parametrize("case", [ref.STRIPS_2, ref.STRIPS_3], ids=["two_rounds", "three_rounds"])
def test_strip_maps(dev, case):
    import insar_unet_ca_amd as iu
    widths, t, rounds = case
    m = ref.strips(widths)
    out = iu.sieve_regions(_t(m, dev), min_area=t, void_value=None)
    _same_sieve(out, ref.sieve(m, t, void_value=None), m, f"strips {widths}")
    assert out["rounds"] == rounds and out["converged"] is True
    one = iu.sieve_regions(_t(m, dev), min_area=t, void_value=None, max_rounds=1)
    _same_sieve(one, ref.sieve(m, t, void_value=None, max_rounds=1), m, f"strips {widths}, one round")
    assert one["rounds"] == 1 and one["converged"] is False
    five = iu.sieve_regions(_t(m, dev), min_area=t, void_value=None, max_rounds=5)          # a second batch of rounds
    _same_sieve(five, ref.sieve(m, t, void_value=None, max_rounds=5), m, f"strips {widths}, five rounds")


def test_concentric_squares(dev):
    import insar_unet_ca_amd as iu
    m = ref.squares(41)
    for conn in (4, 8):
        for t in (50, 200, {1: 130}):
            out = iu.sieve_regions(_t(m, dev), min_area=t, connectivity=conn)
            _same_sieve(out, ref.sieve(m, t, connectivity=conn), m, f"squares, connectivity {conn}, {t}")


def test_three_classes_and_per_class_thresholds(dev):
    import insar_unet_ca_amd as iu
    m = ref.blob_speckle(97, 130, seed=5, classes=3)
    assert set(np.unique(m).tolist()) == {0, 1, 2, 255}
    for t in (20, {1: 30, 2: 12}, [0, 0, 25], {0: 6, 1: 0, 2: 40}):
        out = iu.sieve_regions(_t(m, dev), min_area=t, connectivity=8, return_changed=True)
        want = ref.sieve(m, t, connectivity=8)
        _same_sieve(out, want, m, f"three classes, {t}")
        assert want["absorbed"] > 0
    speck = np.ones((9, 12), dtype=np.uint8)                       # a speck of class 2 inside a class-1 site becomes class 1
    speck[0] = 0
    speck[4, 5] = 2
    out = iu.sieve_regions(_t(speck, dev), min_area={2: 4})
    assert out["mask"][4, 5].item() == 1 and out["changed_pixels"] == 1 and out["absorbed"] == 1


def test_void_values(dev):
    import insar_unet_ca_amd as iu
    m = _map(33, 65)
    for void in (None, 0, 1, 255):
        out = iu.sieve_regions(_t(np.where(m == 255, 7, m) if void is None else m, dev), min_area=11, void_value=void)
        _same_sieve(out, ref.sieve(np.where(m == 255, 7, m) if void is None else m, 11, void_value=void),
                    m, f"void_value {void}")
    with pytest.raises(InsarError, match="class 255"):
        iu.sieve_regions(_t(m, dev), min_area=11, void_value=None)


def test_limits_raise(dev):
    import insar_unet_ca_amd as iu
    m = _t(_map(64, 128), dev)
    n = _sieved(64, 128, 8)["regions_in"]
    with pytest.raises(InsarError, match=f"max_regions={n - 1}"):
        iu.sieve_regions(m, min_area=T2, max_regions=n - 1)
    with pytest.raises(InsarError, match="max_pairs=8"):
        iu.sieve_regions(m, min_area=T2, max_pairs=8)
    _same_sieve(iu.sieve_regions(m, min_area=T2, max_regions=n), _sieved(64, 128, 8), _map(64, 128), "exactly max_regions")


def test_reused_scratch_is_bitwise_reproducible(dev):
    import insar_unet_ca_amd as iu
    m, other = _t(_map(97, 130), dev), _t(ref.blob_speckle(97, 130, seed=77), dev)
    scratch = iu.SieveScratch(97, 130, dev, max_regions=4000, max_pairs=1 << 14, max_rounds=64)
    kw = dict(min_area=T2, max_regions=4000, max_pairs=1 << 14, scratch=scratch, return_changed=True)
    a = iu.sieve_regions(m, **kw)
    iu.sieve_regions(other, min_area=30, connectivity=4, max_regions=4000, max_pairs=1 << 14, scratch=scratch)
    iu.region_adjacency(a["labels_in"], max_pairs=1 << 14, scratch=scratch)
    b = iu.sieve_regions(m, **kw)
    _same_sieve(a, _sieved(97, 130, 8), _map(97, 130), "first call")
    for k in ("mask", "labels_in", "changed"):
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(a["root"], b["root"])
    assert all(a[k] == b[k] for k in ("regions_in", "absorbed", "changed_pixels", "rounds", "converged"))
    with pytest.raises(InsarError, match="scratch of"):
        iu.sieve_regions(m, min_area=T2, scratch=scratch)


@pytest.mark.parametrize("H,W", [(33, 65), (64, 128)])
def test_second_sieve_is_a_no_op(dev, H, W):
    import insar_unet_ca_amd as iu
    first = iu.sieve_regions(_t(_map(H, W), dev), min_area=T2)
    again = iu.sieve_regions(first["mask"], min_area=T2)
    assert again["rounds"] == 0 and again["converged"] is True and again["absorbed"] == 0 and again["changed_pixels"] == 0
    assert torch.equal(again["mask"], first["mask"]) and again["mask"].data_ptr() != first["mask"].data_ptr()
    assert np.array_equal(again["root"], np.arange(again["regions_in"] + 1))


def test_binary_map_equals_label_regions_min_area(dev):
    import insar_unet_ca_amd as iu
    m = np.where(_map(64, 128) == 255, 0, _map(64, 128)).astype(np.uint8)      # binary, no void; every region has a neighbour
    t = _t(m, dev)
    out = iu.sieve_regions(t, min_area={1: 12}, void_value=None)
    reg = iu.label_regions(t, min_area=12)
    assert torch.equal(out["mask"], reg["mask"]) and out["absorbed"] > 0
    assert iu.label_regions(out["mask"])["count"] == reg["count"]


# ---- the scene pipeline ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predictor(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    scene = np.random.default_rng(4).standard_normal((128, 128)).astype(np.float32)
    pred = iu.ScenePredictor(net, tile=64, overlap=8, batch=4, num_classes=2)
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():                                         # split the class map about evenly (tests/test_outlines_gpu.py)
        net.outc.bias[1] += torch.log(p[0] / p[1]).median()
    return pred, scene


def _same(x, y):
    if isinstance(x, torch.Tensor):
        return torch.equal(x, y)
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, np.ndarray):
        return np.array_equal(x, y)
    return x == y


def test_detect_sieves_before_it_labels(dev, predictor):
    import insar_unet_ca_amd as iu
    pred, scene = predictor
    kw = dict(connectivity=4, min_area=2)
    plain = pred.detect(scene, **kw)
    sieve = {1: 20, 0: 8}
    det = pred.detect(scene, sieve=sieve, **kw)
    by_hand = iu.sieve_regions(plain["mask"], min_area=sieve, connectivity=4)
    want = ref.sieve(plain["mask"].cpu().numpy(), sieve, connectivity=4)
    assert np.array_equal(by_hand["mask"].cpu().numpy(), want["mask"]) and want["absorbed"] > 0
    reg = iu.label_regions(by_hand["mask"], plain["conf"], **kw)
    assert torch.equal(det["mask"], plain["mask"]) and torch.equal(det["conf"], plain["conf"])
    assert torch.equal(det["mask_sieved"], by_hand["mask"]) and torch.equal(det["labels"], reg["labels"])
    assert torch.equal(det["mask_clean"], reg["mask"]) and det["count"] == reg["count"] and _same(det["regions"], reg["regions"])
    assert (det["sieve_changed_pixels"], det["sieve_absorbed"], det["sieve_rounds"], det["sieve_converged"]) == \
        (by_hand["changed_pixels"], by_hand["absorbed"], by_hand["rounds"], by_hand["converged"])
    assert set(det) - set(plain) == {"mask_sieved", "sieve_changed_pixels", "sieve_absorbed", "sieve_rounds", "sieve_converged"}
    for form in ({"min_area": sieve}, {"min_area": [8, 20], "max_rounds": 16, "max_pairs": 1 << 15}):
        assert torch.equal(pred.detect(scene, sieve=form, **kw)["labels"], det["labels"])
    conn8 = pred.detect(scene, sieve={"min_area": sieve, "connectivity": 8}, **kw)
    assert torch.equal(conn8["mask_sieved"], iu.sieve_regions(plain["mask"], min_area=sieve, connectivity=8)["mask"])
    print(f"detect: {plain['count']} regions -> {det['count']}, {det['sieve_absorbed']} absorbed in {det['sieve_rounds']} rounds")


def test_detect_without_sieve_is_unchanged(dev, predictor):
    import insar_unet_ca_amd as iu
    pred, scene = predictor
    kw = dict(connectivity=8, min_area=2, outlines=True)
    a, b = pred.detect(scene, **kw), pred.detect(scene, sieve=None, **kw)
    by_hand = dict(pred.predict(scene))
    reg = iu.label_regions(by_hand["mask"], by_hand["conf"], connectivity=8, min_area=2)
    assert a.keys() == b.keys() == {"mask", "conf", "labels", "regions", "count", "mask_clean", "outlines"}
    for k in a:
        assert _same(a[k], b[k]), k
    assert torch.equal(a["labels"], reg["labels"]) and torch.equal(a["mask_clean"], reg["mask"])
    for bad in ("yes", True, {"max_rounds": 3}, {"min_area": 3, "scratch": None}):
        with pytest.raises(InsarError, match="sieve"):
            pred.detect(scene, sieve=bad)
    with pytest.raises(InsarError, match="min_area=-3"):
        pred.detect(scene, sieve=-3)


def test_evaluate_sieves_the_prediction_only(dev, predictor):
    pred, scene = predictor
    gt = ref.blob_speckle(128, 128, seed=9)                       # a ground truth with specks and void of its own
    plain = pred.evaluate(scene, gt, connectivity=8, min_area=2)
    out = pred.evaluate(scene, gt, sieve={1: 20, 0: 8}, connectivity=8, min_area=2)
    det = pred.detect(scene, sieve={1: 20, 0: 8}, connectivity=8, min_area=2)
    assert torch.equal(out["labels"], det["labels"]) and out["sieve_absorbed"] == det["sieve_absorbed"] > 0
    assert out["gt_count"] == plain["gt_count"] and torch.equal(out["gt_labels"], plain["gt_labels"])
    assert _same(out["gt_regions"], plain["gt_regions"])
    assert len(out["score"]["pred_match"]) == out["count"] and len(out["score"]["gt_match"]) == out["gt_count"]
