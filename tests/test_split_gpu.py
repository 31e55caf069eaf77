"""GPU: splitting touching sites (insar_unet_ca_amd/split.py on csrc/split.hip) against the numpy restatement of
tests/split_ref.py (pinned on the prototype's outcomes in tests/test_split_host.py).

Every comparison is exact: the label map, every integer field of the table, cy / cx / mean_conf (the same int64 sums divided in
float64 on both sides), raw_basins, rounds and converged. The canvases are 70 x 150 and 61 x 131: a work-group covers 256
consecutive pixels and a numbering block 1024, so every shape straddles both, ragged against every power of two."""
import functools

import numpy as np
import pytest
import torch

from insar_unet_ca_amd._lib import InsarError
from tests import split_ref as sr

pytestmark = pytest.mark.gpu
INT_FIELDS = ("id", "cls", "area", "y0", "x0", "y1", "x1", "parent", "peak", "peak_y", "peak_x", "saddle")
FLOAT_FIELDS = ("cy", "cx")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _compare(out, ref, what=""):
    assert out["labels"].dtype == torch.int32
    got = (out["raw_basins"], out["count"], out["rounds"], out["converged"])
    want = (ref["raw_basins"], ref["count"], ref["rounds"], ref["converged"])
    print(f"{what}: (raw basins, pieces, rounds, converged) = {got}, restatement {want}")
    assert got == want, what
    labels = out["labels"].cpu().numpy()
    assert np.array_equal(labels, ref["labels"]), f"{what}: {(labels != ref['labels']).sum()} labels differ"
    r, o = out["regions"], ref["regions"]
    with_conf = "mean_conf" in o
    assert ("mean_conf" in r) == with_conf
    for f in INT_FIELDS + FLOAT_FIELDS + (("mean_conf",) if with_conf else ()):
        assert r[f].shape == (ref["count"],) and np.array_equal(r[f], o[f]), f"{what}: {f}"
    assert r["area"].dtype == np.int64 and r["cy"].dtype == np.float64


def _run(dev, m, *, height=None, mask=None, conf=None, **kw):
    import insar_unet_ca_amd as iu
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return iu.split_regions(t(m), height=t(height), mask=t(mask), conf=t(conf), **kw)


@functools.lru_cache(maxsize=None)
def _prototype(name, H, W):
    case = {c[0]: c for c in sr.PROTOTYPE_CASES}[name]
    m = case[1](H, W)
    return m, sr.split_oracle(m, min_depth=case[2])


@pytest.mark.parametrize("H,W", [(70, 150), (61, 131)])
@pytest.mark.parametrize("case", sr.PROTOTYPE_CASES, ids=[c[0] for c in sr.PROTOTYPE_CASES])
def test_prototype_shapes(dev, case, H, W):
    name, _, min_depth, raw, pieces, rounds = case
    m, ref = _prototype(name, H, W)
    out = _run(dev, m, min_depth=min_depth)
    _compare(out, ref, f"{name} {H} x {W}")
    assert (out["raw_basins"], out["count"], out["rounds"]) == (raw, pieces, rounds)


def test_ridge_plateau_across_work_groups(dev):
    """A horizontal bar 9 x 300: its ridge is one plateau 292 pixels long, over several work-groups and tiles."""
    m = np.zeros((21, 320), dtype=np.int32)
    m[6:15, 10:310] = 1
    for min_depth in (0.0, 1.0):
        _compare(_run(dev, m, min_depth=min_depth), sr.split_oracle(m, min_depth=min_depth), f"bar, min_depth {min_depth}")


@functools.lru_cache(maxsize=None)
def _random_case(seed):
    return sr.random_labels(96, 130, seed)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("min_depth", [0, 1, 3])
def test_random_labels_with_small_integer_heights(dev, seed, min_depth):
    m, h = _random_case(seed)
    ref = sr.split_oracle(m, height=h, squared=False, min_depth=min_depth)
    out = _run(dev, m, height=h, squared=False, min_depth=min_depth)
    _compare(out, ref, f"random {seed}, min_depth {min_depth}")
    assert out["raw_basins"] > out["count"] >= 1


def test_random_labels_with_distance_heights(dev):
    m, _ = _random_case(2)
    for min_depth in (0.0, 1.0, 4096.0):
        _compare(_run(dev, m, min_depth=min_depth), sr.split_oracle(m, min_depth=min_depth), f"random 2, min_depth {min_depth}")
    whole = _run(dev, m, min_depth=4096.0)["labels"].cpu().numpy()
    assert np.array_equal(whole, sr.components_by_first_pixel(m))      # label_regions's numbering where nothing is cut


def test_numbering_scan_runs_a_second_pass(dev):
    """1030 x 1024 pixels are 1030 numbering blocks, and the scan of their counts takes 1024 per pass: the pieces of the last six
    blocks get their ids from the carry of the first pass, and the header its count. One-pixel sites 4099 pixels apart (four rows
    and three columns, never neighbours) with a given height are a piece each, numbered in row-major order."""
    H, W = 1030, 1024
    at = np.arange(5, H * W, 4099)
    m = np.zeros(H * W, dtype=np.int32)
    m[at] = 1
    out = _run(dev, m.reshape(H, W), height=m.reshape(H, W), squared=False, min_depth=0, max_pairs=1024)
    want = np.zeros(H * W, dtype=np.int32)
    want[at] = np.arange(1, at.size + 1)
    assert at[-1] // 1024 >= 1024 and (out["count"], out["raw_basins"]) == (at.size, at.size)
    assert np.array_equal(out["labels"].cpu().numpy().ravel(), want)
    r = out["regions"]
    assert np.array_equal(r["id"], np.arange(1, at.size + 1)) and (r["area"] == 1).all() and (r["parent"] == 1).all()
    assert np.array_equal(r["peak_y"], at // W) and np.array_equal(r["peak_x"], at % W)


@pytest.mark.parametrize("shape", [(1, 1), (1, 200), (200, 1)])
def test_degenerate_shapes(dev, shape):
    rng = np.random.default_rng(sum(shape))
    m = (rng.random(shape) < 0.7).astype(np.int32) * rng.integers(1, 3, size=shape).astype(np.int32)
    h = rng.integers(0, 4, size=shape).astype(np.int32)
    _compare(_run(dev, m, min_depth=0.5), sr.split_oracle(m, min_depth=0.5), f"{shape}, distance heights")
    _compare(_run(dev, m, height=h, min_depth=1), sr.split_oracle(m, height=h, min_depth=1), f"{shape}, given heights")


def test_all_background_and_one_label_over_the_whole_map(dev):
    zero = np.zeros((40, 70), dtype=np.int32)
    out = _run(dev, zero)
    _compare(out, sr.split_oracle(zero), "all background")
    assert out["count"] == 0 and out["raw_basins"] == 0 and not out["labels"].any()
    full = np.full((40, 70), 5, dtype=np.int32)
    out = _run(dev, full)
    _compare(out, sr.split_oracle(full), "one label everywhere")
    assert out["count"] == 1 and out["regions"]["peak"][0] == sr.FAR and out["regions"]["parent"][0] == 5


def test_regions_on_the_image_border_and_bounded_heights(dev):
    m = np.zeros((70, 150), dtype=np.int32)
    sr.disc(m, 0, 30, 20, 1)
    sr.disc(m, 0, 60, 20, 1)
    sr.disc(m, 69, 149, 25, 2)
    m[30:40, 0:50] = 3
    m[35:70, 0:8] = 3
    for kw in (dict(min_depth=1.0), dict(min_depth=1.0, max_distance=4), dict(min_depth=0.0, max_distance=4)):
        out = _run(dev, m, **kw)
        _compare(out, sr.split_oracle(m, **kw), f"border regions {kw}")
        if "max_distance" in kw:
            assert out["regions"]["peak"].max() == 16             # the plateau of clamped heights


def test_max_rounds_and_converged(dev):
    m, ref = _prototype("three_discs_deep", 61, 131)
    one = _run(dev, m, min_depth=10.0, max_rounds=1)
    _compare(one, sr.split_oracle(m, min_depth=10.0, max_rounds=1), "chain, one round")
    assert one["converged"] is False and one["rounds"] == 1
    full = _run(dev, m, min_depth=10.0)
    assert full["converged"] is True and full["rounds"] == 2 and full["count"] == 1
    five = _run(dev, m, min_depth=10.0, max_rounds=5)             # a second batch of rounds
    _compare(five, ref, "chain, five rounds")


def test_limits_raise(dev):
    m = sr.speckle_labels(64, 96, 7)
    with pytest.raises(InsarError, match="max_pairs=8"):
        _run(dev, m, max_pairs=8)
    with pytest.raises(InsarError, match="max_regions=2"):
        _run(dev, m, max_regions=2)
    with pytest.raises(InsarError, match="negative"):
        _run(dev, m, height=np.full(m.shape, -1, dtype=np.int32))
    _compare(_run(dev, m, max_pairs=4096), sr.split_oracle(m), "speckle")


def test_reused_scratch_is_bitwise_reproducible(dev):
    import insar_unet_ca_amd as iu
    m, h = _random_case(1)
    other, _ = _random_case(0)
    scratch = iu.SplitScratch(96, 130, dev, max_regions=2000, max_pairs=5000, max_rounds=64)
    kw = dict(squared=False, min_depth=1, max_regions=2000, max_pairs=5000, scratch=scratch)
    a = _run(dev, m, height=h, **kw)
    _run(dev, other, min_depth=0.0, max_regions=2000, max_pairs=5000, scratch=scratch)          # another map through the scratch
    b = _run(dev, m, height=h, **kw)
    assert torch.equal(a["labels"], b["labels"]) and (a["rounds"], a["raw_basins"]) == (b["rounds"], b["raw_basins"])
    for f in a["regions"]:
        assert np.array_equal(a["regions"][f], b["regions"][f]), f
    with pytest.raises(InsarError, match="scratch of"):
        _run(dev, m, height=h, squared=False, min_depth=1, scratch=scratch)


def test_mask_and_conf_give_cls_and_mean_conf(dev):
    m, h = _random_case(0)
    rng = np.random.default_rng(11)
    mask = np.where(m > 0, 1 + m % 3, 0).astype(np.uint8)
    conf = (rng.random(m.shape) * 1.2 - 0.1).astype(np.float32)   # some outside 0..1: clamped
    ref = sr.split_oracle(m, height=h, min_depth=1, mask=mask, conf=conf)
    out = _run(dev, m, height=h, min_depth=1, mask=mask, conf=conf)
    _compare(out, ref, "mask and conf")
    assert set(out["regions"]["cls"].tolist()) <= {1, 2, 3} and len(set(out["regions"]["cls"].tolist())) > 1


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


def test_detect_splits_and_outlines_follow_the_pieces(dev, predictor):
    import insar_unet_ca_amd as iu
    pred, scene = predictor
    kw = dict(connectivity=8, min_area=2)
    plain = pred.detect(scene, **kw)
    ref = sr.split_oracle(plain["labels"].cpu().numpy(), mask=plain["mask_clean"].cpu().numpy(), conf=plain["conf"].cpu().numpy(),
                          min_depth=1.0)
    det = pred.detect(scene, split=1.0, outlines=True, simplify=1.0, **kw)
    _compare({**det, "raw_basins": ref["raw_basins"], "rounds": det["split_rounds"], "converged": det["split_converged"]}, ref,
             "detect(split=1.0)")
    assert det["count"] >= plain["count"] and torch.equal(det["mask_clean"], plain["mask_clean"])
    assert np.isin(det["regions"]["parent"], plain["regions"]["id"]).all() and len(det["regions"]["perimeter"]) == det["count"]
    H, W = det["labels"].shape
    res = iu.rasterise_polygons(iu.pack_polygons(iu.to_polygons(det["outlines"])), H, W, dtype=torch.int32, device=dev)
    assert int(res["overlap_pixels"]) == 0
    exact = pred.detect(scene, split={"min_depth": 1.0}, outlines=True, simplify=0, **kw)
    assert torch.equal(exact["labels"], det["labels"])
    res = iu.rasterise_polygons(iu.pack_polygons(iu.to_polygons(exact["outlines"])), H, W, dtype=torch.int32, device=dev)
    assert int(res["overlap_pixels"]) == 0 and torch.equal(res["labels"], det["labels"])
    print(f"detect: {plain['count']} regions -> {det['count']} pieces in {det['split_rounds']} rounds")


def test_detect_without_split_is_unchanged(dev, predictor):
    pred, scene = predictor
    kw = dict(connectivity=8, min_area=2, outlines=True)
    a, b = pred.detect(scene, **kw), pred.detect(scene, split=None, **kw)
    assert a.keys() == b.keys() and "split_rounds" not in a

    def same(x, y):
        if isinstance(x, torch.Tensor):
            return torch.equal(x, y)
        if isinstance(x, dict):
            return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
        if isinstance(x, np.ndarray):
            return np.array_equal(x, y)
        return x == y
    for k in a:
        assert same(a[k], b[k]), k
    with pytest.raises(InsarError, match="split"):
        pred.detect(scene, split="yes")


def test_evaluate_scores_the_pieces(dev, predictor):
    pred, scene = predictor
    gt = (np.random.default_rng(9).random((128, 128)) < 0.3).astype(np.uint8)
    out = pred.evaluate(scene, gt, split=0.5, connectivity=8, min_area=2)
    plain = pred.evaluate(scene, gt, connectivity=8, min_area=2)
    assert out["count"] >= plain["count"] and "split_rounds" in out
    assert len(out["score"]["pred_match"]) == out["count"] == len(out["regions"]["id"])
    assert out["gt_count"] == plain["gt_count"] and torch.equal(out["gt_labels"], plain["gt_labels"])
