"""No GPU: the numpy restatement of the hysteresis rule (tests/hysteresis_ref.py) pinned on hand-built cases, the key order, the
host-only entry points and argument checks of insar_unet_ca_amd/hysteresis.py and csrc/hysteresis.hip, and the condition that
the maps of the GPU comparison (tests/test_hysteresis_gpu.py) exercise what they are there for."""
import numpy as np
import pytest
import torch

from insar_unet_ca_amd import _lib
from insar_unet_ca_amd import hysteresis as hy
from insar_unet_ca_amd._lib import InsarError
from tests import hysteresis_ref as ref


def _f(rows):
    return np.array(rows, dtype=np.float32)


# ---- the rule on hand-built maps -------------------------------------------------------------------------------------------
def test_a_ring_of_low_pixels_with_one_seed():
    s = np.zeros((7, 7), dtype=np.float32)
    s[1:6, 1:6] = 0.5
    s[2:5, 2:5] = 0.0                                             # a ring, one pixel wide
    s[5, 5] = 0.9                                                 # its one seed, the last pixel in row-major order
    s[0, 6] = 0.5                                                 # a lone low pixel that touches the ring only diagonally... not at all
    res = ref.hysteresis(s, 0.25, 0.75, connectivity=4)
    assert res["count"] == 1 and res["candidates"] == 2 and res["unseeded"] == 1
    r = res["regions"]
    assert r["area"].tolist() == [16] and r["n_seed"].tolist() == [1] and r["peak"].tolist() == [np.float32(0.9)]
    assert (r["peak_y"].tolist(), r["peak_x"].tolist()) == ([5], [5]) and res["root"].tolist() == [8]
    assert (r["y0"][0], r["x0"][0], r["y1"][0], r["x1"][0]) == (1, 1, 6, 6)
    assert res["labels"][0, 6] == 0 and res["mask"][0, 6] == 0 and res["conf"][0, 6] == np.float32(0.5)
    assert (res["labels"] == 1).sum() == 16 and res["mask"].sum() == 16
    assert r["mean_conf"][0] == (15 * ref.quantise_conf(0.5) + ref.quantise_conf(np.float32(0.9))) / (16.0 * ref.CONF_SCALE)
    assert ref.hysteresis(s, 0.25, 0.95)["count"] == 0            # no pixel reaches 0.95: extent alone makes no site


def test_two_classes_touching_with_a_seed_in_only_one():
    s = np.zeros((3, 4, 8), dtype=np.float32)
    s[0] = 0.5
    s[1, 1:3, 0:4] = 0.4                                          # class 1: faint, no seed
    s[2, 1:3, 4:8] = 0.4                                          # class 2 touches it
    s[2, 2, 7] = 0.8
    res = ref.hysteresis(s, 0.3, 0.7)
    assert res["cand"][1].tolist() == [1, 1, 1, 1, 2, 2, 2, 2]
    assert res["count"] == 1 and res["candidates"] == 2 and res["regions"]["cls"].tolist() == [2]
    assert res["mask"][1].tolist() == [0, 0, 0, 0, 2, 2, 2, 2] and res["labels"][1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    # the background plane never takes part: p(background) = 0.5 beats every class here, and the classes are candidates still
    assert (res["cand"][1:3] > 0).all() and (res["cand"][0] == 0).all()
    # per-class thresholds and a class subset
    assert ref.hysteresis(s, {1: 0.3, 2: 0.3}, {1: 0.4, 2: 0.9})["regions"]["cls"].tolist() == [1]
    assert ref.hysteresis(s, 0.3, 0.4, classes=[1])["regions"]["cls"].tolist() == [1]
    assert ref.hysteresis(s, 0.3, 0.4, classes=[1])["cand"].max() == 1
    # where two classes qualify the greater score wins, and a tie goes to the smaller class
    t = np.zeros((3, 1, 3), dtype=np.float32)
    t[1, 0], t[2, 0] = [0.5, 0.6, 0.5], [0.5, 0.5, 0.75]
    assert ref.candidates(t, 0.25, 0.75)[0].tolist() == [[1, 1, 2]]


def test_a_diagonal_link_at_a_tile_corner():
    s = np.zeros((34, 66), dtype=np.float32)
    s[30:32, 62:64] = 0.5                                         # ends at (31, 63), the last pixel of labelling tile (0, 0)
    s[32:34, 64:66] = 0.5                                         # starts at (32, 64), the first pixel of tile (1, 1)
    s[33, 65] = 1.0
    eight, four = ref.hysteresis(s, 0.25, 0.75, connectivity=8), ref.hysteresis(s, 0.25, 0.75, connectivity=4)
    assert eight["count"] == 1 and eight["regions"]["area"].tolist() == [8] and ref.far_seeded(eight) == [1]
    assert four["count"] == 1 and four["candidates"] == 2 and four["regions"]["area"].tolist() == [4]
    assert four["root"].tolist() == [32 * 66 + 64] and ref.far_seeded(four) == []


def test_equality_at_both_thresholds():
    s = _f([[0.25, 0.25, 0.0, 0.24999999, 0.75], [0.0, 0.0, 0.0, 0.0, 0.0], [0.25, 0.74999994, 0.0, 0.75, 0.0]])
    res = ref.hysteresis(s, 0.25, 0.75, connectivity=4)
    assert res["cand"].tolist() == [[1, 1, 0, 0, 1], [0, 0, 0, 0, 0], [1, 1, 0, 1, 0]]
    assert res["seed"].tolist() == [[False, False, False, False, True], [False] * 5, [False, False, False, True, False]]
    assert res["count"] == 2 and res["candidates"] == 4 and res["root"].tolist() == [4, 13]
    same = ref.hysteresis(s, 0.25, 0.25, connectivity=4)          # low == high: every candidate is a seed
    assert same["count"] == same["candidates"] == 4 and same["regions"]["n_seed"].tolist() == same["regions"]["area"].tolist()


def test_nan_pixels_are_no_candidates():
    s = _f([[0.5, np.nan, 0.5], [np.nan, np.nan, np.nan], [0.9, 0.5, np.nan]])
    res = ref.hysteresis(s, -1.0, 0.75)
    assert res["cand"].tolist() == [[1, 0, 1], [0, 0, 0], [1, 1, 0]] and res["count"] == 1
    assert not np.isnan(res["conf"]).any() and res["conf"][1, 1] == 0
    assert (res["regions"]["peak_y"][0], res["regions"]["peak_x"][0]) == (2, 0)
    v = np.ones((3, 3), dtype=np.uint8)
    v[2, 0] = 0                                                   # an invalid seed is no seed
    assert ref.hysteresis(s, -1.0, 0.75, valid=v)["count"] == 0 and ref.hysteresis(s, -1.0, 0.75, valid=v)["conf"][2, 0] == 0


def test_a_peak_tie_goes_to_the_first_pixel_and_min_seeds_counts():
    s = _f([[0.5, 0.875, 0.5, 0.875], [0.875, 0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 0.0], [0.5, 0.8, 0.5, 0.0]])
    res = ref.hysteresis(s, 0.25, 0.75)
    r = res["regions"]
    assert r["n_seed"].tolist() == [3, 1] and r["peak"].tolist() == [np.float32(0.875), np.float32(0.8)]
    assert (r["peak_y"].tolist(), r["peak_x"].tolist()) == ([0, 3], [1, 1])
    two = ref.hysteresis(s, 0.25, 0.75, min_seeds=2)
    assert two["count"] == 1 and two["candidates"] == 2 and two["unseeded"] == 1 and two["regions"]["n_seed"].tolist() == [3]
    assert ref.hysteresis(s, 0.25, 0.75, min_seeds=4)["count"] == 0
    big = ref.hysteresis(s, 0.25, 0.75, min_area=4)               # min_area comes before the seed rule
    assert big["count"] == 1 and big["candidates"] == 1 and big["unseeded"] == 0
    neg = ref.hysteresis(_f([[-0.5, -0.25, -0.5, -0.0, 0.0]]) - np.float32(0), -1.0, -0.3)      # negative scores: no clamp in the peak
    assert neg["regions"]["peak"].tolist() == [0.0] and neg["regions"]["peak_x"].tolist() == [4]
    assert neg["regions"]["mean_conf"].tolist() == [0.0]          # ... but the quantised mean clamps at 0, as label_regions' does


def test_raising_high_only_removes_regions():
    s = ref.blob_scores(33, 65, 7, 2)
    prev = None
    for high in (0.25, 0.5, 0.75, 1.0):
        res = ref.hysteresis(s, 0.25, high)
        sets = {frozenset(np.flatnonzero(res["labels"].ravel() == k).tolist()) for k in range(1, res["count"] + 1)}
        assert prev is None or sets <= prev
        prev = sets


# ---- the key order ---------------------------------------------------------------------------------------------------------
def test_ordered_u32_sorts_like_float32():
    tiny = np.float32(1e-45)
    v = _f([0.0, -0.0, tiny, -tiny, np.float32(1.1754942e-38), -np.float32(1.1754942e-38), 1.0, -1.0, 0.75, 0.74999994, 3.4e38, -3.4e38,
            np.inf, -np.inf, 0.25, 1 / 64])
    for fn in (ref.ordered_u32, hy.ordered_u32):
        k = fn(v)
        assert k.dtype == np.uint32
        order = np.argsort(k, kind="stable")
        assert np.array_equal(v[order], np.sort(v)) or np.array_equal(np.abs(v[order]), np.abs(np.sort(v)))
        s = v[order]
        assert (np.diff(s) >= 0).all() and (np.diff(k[order].astype(np.int64)) > 0).all()     # strictly: -0.0 sits below 0.0
        assert k[1] + 1 == k[0] and k[np.argmax(v)] == k.max() and k[np.argmin(v)] == k.min()
    assert np.array_equal(hy.from_ordered_u32(hy.ordered_u32(v)).view(np.uint32), v.view(np.uint32))
    assert np.array_equal(ref.ordered_u32(v), hy.ordered_u32(v))


# ---- host-only entry points ------------------------------------------------------------------------------------------------
def test_scratch_bytes_is_host_arithmetic():
    sb, tb = hy.scratch_bytes(100, 130, 1000)
    assert sb == 16 * 1001 + (4 * 1001 + 15) // 16 * 16 and tb == 80 * 1001 and sb % 16 == 0
    assert hy.scratch_bytes(1, 1, 1) == (32 + 16, 160)
    assert hy.HYST_DTYPE.itemsize == 80 and hy.HYST_DTYPE.fields["n_seed"][1] == 64 and hy.HYST_DTYPE.fields["peak_key"][1] == 72
    for bad in ((0, 5, 1), (5, 0, 1), (1 << 16, 1 << 15, 1), (4, 4, 0), (4, 4, -3)):
        with pytest.raises(InsarError):
            hy.scratch_bytes(*bad)
    assert hy.LAUNCHES == 12


def test_entry_points_refuse_bad_arguments_without_a_device():
    A = 4096                                                      # a 16-byte aligned address that is never dereferenced
    bad = [
        ("insar_hyst_classify", (0, 1, 4, 4, A, 0, A, A, None), "null pointer"),
        ("insar_hyst_classify", (A, 1, 4, 4, 0, 0, A, A, None), "null pointer"),
        ("insar_hyst_classify", (A, 1, 4, 4, A, 0, 0, A, None), "null pointer"),
        ("insar_hyst_classify", (A, 1, 4, 4, A, 0, A, 0, None), "null pointer"),
        ("insar_hyst_classify", (A + 2, 1, 4, 4, A, 0, A, A, None), "not 4-byte aligned"),
        ("insar_hyst_classify", (A, 0, 4, 4, A, 0, A, A, None), "0 planes"),
        ("insar_hyst_classify", (A, 256, 4, 4, A, 0, A, A, None), "256 planes"),
        ("insar_hyst_classify", (A, 1, 0, 4, A, 0, A, A, None), "empty scene"),
        ("insar_hyst_classify", (A, 1, 1 << 16, 1 << 15, A, 0, A, A, None), "2\\^31"),
        ("insar_hyst_seeds", (0, A, A, A, 4, 4, 8, A, None), "null pointer"),
        ("insar_hyst_seeds", (A, 0, A, A, 4, 4, 8, A, None), "null pointer"),
        ("insar_hyst_seeds", (A, A, 0, A, 4, 4, 8, A, None), "null pointer"),
        ("insar_hyst_seeds", (A, A, A, 0, 4, 4, 8, A, None), "null pointer"),
        ("insar_hyst_seeds", (A, A, A, A, 4, 4, 8, 0, None), "null pointer"),
        ("insar_hyst_seeds", (A, A, A, A, 4, 4, 8, A + 8, None), "not 16-byte aligned"),
        ("insar_hyst_seeds", (A, A, A, A, 4, 4, 0, A, None), "max_regions 0"),
        ("insar_hyst_seeds", (A, A, A, A, 4, -1, 8, A, None), "empty scene"),
        ("insar_hyst_keep", (0, 1, 8, A, 2 * A, None), "null pointer"),
        ("insar_hyst_keep", (A, 1, 8, 0, 2 * A, None), "null pointer"),
        ("insar_hyst_keep", (A, 1, 8, A, 0, None), "null pointer"),
        ("insar_hyst_keep", (A, 0, 8, A, 2 * A, None), "min_seeds 0"),
        ("insar_hyst_keep", (A, 1, 0, A, 2 * A, None), "max_regions 0"),
        ("insar_hyst_keep", (A, 1, 8, 2 * A, A, None), "must not be the region table"),
        ("insar_hyst_apply", (0, 4, 4, 8, A, A, A, None), "null pointer"),
        ("insar_hyst_apply", (A, 4, 4, 8, 0, A, A, None), "null pointer"),
        ("insar_hyst_apply", (A, 4, 4, 8, A, 0, A, None), "null pointer"),
        ("insar_hyst_apply", (A, 4, 4, 8, A, A, 0, None), "null pointer"),
        ("insar_hyst_apply", (A, 4, 4, 8, A, A + 2, A, None), "not 4-byte aligned"),
        ("insar_hyst_apply", (A, 0, 4, 8, A, A, A, None), "empty scene"),
        ("insar_hyst_apply", (A, 4, 4, 0, A, A, A, None), "max_regions 0"),
    ]
    for name, args, msg in bad:
        with pytest.raises(InsarError, match=msg):
            _lib.call(name, *args)
    import ctypes
    cell = ctypes.c_int64(0)
    with pytest.raises(InsarError, match="null pointer"):
        _lib.call("insar_hyst_scratch_bytes", 4, 4, 8, None, ctypes.byref(cell))


# ---- Python arguments ------------------------------------------------------------------------------------------------------
def test_threshold_words():
    w = hy.threshold_words(0.25, 0.75, None, 3)
    assert w.dtype == np.float32 and w.shape == (512,)
    assert w[1:3].tolist() == [0.25, 0.25] and w[257:259].tolist() == [0.75, 0.75] and np.isnan(np.delete(w, [1, 2, 257, 258])).all()
    w = hy.threshold_words({1: 0.1, 2: 0.2}, [9, 0.5, 0.2], [2], 3)
    assert w[2] == np.float32(0.2) and w[258] == np.float32(0.2) and np.isnan(w[1]) and np.isnan(w[257])
    assert hy.threshold_words(np.float32(0.5), 1, (1,), 2)[[1, 257]].tolist() == [0.5, 1.0]


def test_every_argument_error_is_raised_by_name():
    s2, s3 = torch.zeros(6, 8), torch.zeros(3, 6, 8)
    bad = [
        (dict(score=np.zeros((6, 8), np.float32)), "score must be a torch tensor"),
        (dict(score=s2.double()), "score must be"),
        (dict(score=s2[None, None]), "score must be"),
        (dict(score=s2.t()), "score must be"),
        (dict(score=torch.zeros(0, 8)), "need H, W >= 1"),
        (dict(score=s2[None]), "a 3-D score needs the background plane"),
        (dict(score=torch.zeros(257, 1, 1)), "a 3-D score needs the background plane"),
        (dict(low=0.8, high=0.2), r"low\[1\]=.*> high\[1\]"),
        (dict(low=float("nan")), r"low\[1\]=nan"),
        (dict(high=float("inf")), r"high\[1\]=inf"),
        (dict(low="x"), "low='x'"),
        (dict(low=True), "low=True"),
        (dict(score=s3, low={3: 0.1}), "low: class=3"),
        (dict(score=s3, low={1: 0.1}), r"low\[2\]=nan"),
        (dict(score=s3, high={1: 0.9, 2: "a"}), r"high\[2\]='a'"),
        (dict(score=s3, low=[0.1, 0.2]), "low: a sequence indexed by class has 3 entries"),
        (dict(score=s3, low=[0, 0.5, 0.6], high=[0, 0.9, 0.5]), r"low\[2\]=.*> high\[2\]"),
        (dict(classes=[0]), "classes: class=0"),
        (dict(classes=[2]), "classes: class=2"),
        (dict(score=s3, classes=[3]), "classes: class=3"),
        (dict(score=s3, classes=[1, 1]), "named twice"),
        (dict(classes=5), "classes=5"),
        (dict(valid=torch.ones(6, 8)), "valid must be"),
        (dict(valid=torch.ones(6, 9, dtype=torch.uint8)), r"valid \(6, 9\): expected \(6, 8\) for score"),
        (dict(valid=np.ones((6, 8), np.uint8)), "valid must be a torch tensor"),
        (dict(connectivity=6), "connectivity=6"),
        (dict(min_area=0), "min_area=0"),
        (dict(min_seeds=0), "min_seeds=0"),
        (dict(min_seeds=1.5), "min_seeds=1.5"),
        (dict(max_regions=0), "max_regions=0"),
        (dict(scratch=object()), "scratch must be a HysteresisScratch"),
        (dict(), "score must be a ROCm tensor"),                  # the device comes last
        (dict(score=s3), "score must be a ROCm tensor"),
    ]
    for kw, msg in bad:
        args = dict(score=s2, low=0.25, high=0.75)
        args.update(kw)
        score, low, high = args.pop("score"), args.pop("low"), args.pop("high")
        with pytest.raises(InsarError, match=msg):
            hy.hysteresis_regions(score, low, high, **args)


def test_detect_refuses_what_hysteresis_replaces_before_it_predicts():
    import insar_unet_ca_amd as iu
    pred = iu.ScenePredictor.__new__(iu.ScenePredictor)           # no model: every refusal below comes before `predict`
    scene = np.zeros((64, 64), dtype=np.float32)
    for kw, msg in [(dict(hysteresis=(0.2, 0.8), min_conf=0.5), "min_conf next to hysteresis"),
                    (dict(hysteresis=(0.2, 0.8), sieve=16), "sieve next to hysteresis.*different maps"),
                    (dict(hysteresis=0.5), "hysteresis: \\(low, high\\) or a dict"),
                    (dict(hysteresis=(0.1, 0.2, 0.3)), "hysteresis: \\(low, high\\) or a dict"),
                    (dict(hysteresis={"low": 0.2}), "needs 'low' and 'high'"),
                    (dict(hysteresis={"low": 0.2, "high": 0.8, "valid": None}), "'valid' is detect's to give"),
                    (dict(hysteresis=(0.2, 0.8), foo=1), "'foo' next to hysteresis")]:
        with pytest.raises(InsarError, match=msg):
            pred.detect(scene, **kw)


def test_exports():
    import insar_unet_ca_amd as iu
    assert iu.hysteresis_regions is hy.hysteresis_regions and iu.HysteresisScratch is hy.HysteresisScratch
    assert "hysteresis_regions" in iu.__all__ and "HysteresisScratch" in iu.__all__


# ---- a condition, not a measurement: the maps of the GPU comparison hold what it is there to compare -------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("H,W", [s for s in ref.SHAPES if s[0] * s[1] >= 33 * 65])
def test_the_gpu_cases_cannot_pass_vacuously(H, W, K, conn):
    res = ref.hysteresis(ref.blob_scores(H, W, H * 1000 + W, K), ref.LOW, ref.HIGH, connectivity=conn)
    far = ref.far_seeded(res)
    print(f"{H} x {W}, K {K}, connectivity {conn}: {res['count']} kept of {res['candidates']}, {res['unseeded']} without a seed, "
          f"{len(far)} seeded from another tile only")
    assert res["count"] >= 1                                      # a kept region
    assert res["unseeded"] >= 1                                   # a component dropped only for lack of a seed
    assert len(far) >= 1                                          # a kept region none of whose seeds lies in its root's tile
    with np.errstate(invalid="ignore"):
        s = ref.blob_scores(H, W, H * 1000 + W, K)
        assert (s == np.float32(ref.LOW)).any() and (s == np.float32(ref.HIGH)).any() and np.isnan(s).any()
