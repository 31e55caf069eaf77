"""CPU-only: the numpy restatement of the splitting rule (tests/split_ref.py) on the prototype's outcomes and its guarantees
(the fixed point, whole regions in label_regions's numbering), and what insar_unet_ca_amd/split.py decides without a device:
argument validation, exports, the ABI version and the scratch arithmetic."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from insar_unet_ca_amd import _lib
from insar_unet_ca_amd import split as sp
from insar_unet_ca_amd._lib import InsarError
from tests import split_ref as sr


@pytest.mark.parametrize("H,W", [(70, 150), (61, 131)])
@pytest.mark.parametrize("case", sr.PROTOTYPE_CASES, ids=[c[0] for c in sr.PROTOTYPE_CASES])
def test_prototype_outcomes(case, H, W):
    name, build, min_depth, raw, pieces, rounds = case
    m = build(H, W)
    assert not (m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any()), "the shape must not touch the canvas border"
    out = sr.split_oracle(m, min_depth=min_depth)
    assert (out["raw_basins"], out["count"], out["rounds"], out["converged"]) == (raw, pieces, rounds, True)
    assert ((out["labels"] > 0) == (m > 0)).all() and out["labels"].max() == pieces
    if min_depth == 4.0:                                          # "for min_depth <= 4": the same partition below it
        low = sr.split_oracle(m, min_depth=1.0)
        assert np.array_equal(low["labels"], out["labels"]) and low["rounds"] == rounds


def test_chain_needs_two_rounds():
    m = sr.discs_map(61, 131, sr.CHAIN3)
    one = sr.split_oracle(m, min_depth=10.0, max_rounds=1)
    assert (one["rounds"], one["converged"]) == (1, False) and one["count"] > 1
    full = sr.split_oracle(m, min_depth=10.0)
    assert (full["rounds"], full["converged"], full["count"]) == (2, True, 1)


def _assert_fixed_point(out, squared, min_depth):
    T = sr.threshold(min_depth, squared)
    r = out["regions"]
    for peak, saddle in zip(r["peak"].tolist(), r["saddle"].tolist()):
        assert saddle <= peak
        if saddle >= 0:
            assert sr.depth(peak, saddle, squared) > T, (peak, saddle, T)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("min_depth", [0, 1, 3])
def test_fixed_point_on_random_heights(seed, min_depth):
    m, h = sr.random_labels(48, 66, seed)
    out = sr.split_oracle(m, height=h, min_depth=min_depth)
    assert out["converged"]
    _assert_fixed_point(out, False, min_depth)
    # the pieces partition the foreground, each inside one input label, numbered by first pixel
    assert ((out["labels"] > 0) == (m > 0)).all()
    r = out["regions"]
    assert np.array_equal(r["parent"], m.ravel()[r["first"]]) and (np.diff(r["first"]) > 0).all()
    for i, parent in zip(r["id"].tolist(), r["parent"].tolist()):
        assert (m[out["labels"] == i] == parent).all()
    assert int(r["area"].sum()) == int((m > 0).sum())


@pytest.mark.parametrize("seed", [3, 4])
def test_fixed_point_on_distance_heights(seed):
    m, _ = sr.random_labels(48, 66, seed)
    for min_depth in (0.0, 0.5, 2.0):
        out = sr.split_oracle(m, min_depth=min_depth)
        assert out["converged"]
        _assert_fixed_point(out, True, min_depth)


@pytest.mark.parametrize("seed", [5, 6])
def test_a_large_min_depth_returns_the_regions_whole(seed):
    m, h = sr.random_labels(48, 66, seed)
    whole = sr.components_by_first_pixel(m)
    for kw in (dict(min_depth=4096.0), dict(height=h, min_depth=7)):
        out = sr.split_oracle(m, **kw)
        assert out["converged"] and np.array_equal(out["labels"], whole), kw
        assert (out["regions"]["saddle"] == -1).all()
    # an input that is already numbered so comes back as it is
    assert np.array_equal(sr.split_oracle(whole, min_depth=4096.0)["labels"], whole)


def test_depth_is_sixteenths_of_a_pixel_in_64_bits():
    assert sr.depth(400, 100, True) == 160 and sr.depth(sr.FAR, 0, True) == math.isqrt(256 * sr.FAR) > 1 << 19
    assert sr.depth(9, 4, False) == 5
    assert sr.threshold(1.0, True) == 16 and sr.threshold(0.03125, True) == 0 and sr.threshold(0.09375, True) == 2     # half to even
    assert sr.threshold(3, False) == 3


def test_bounded_heights_take_far_as_r_squared():
    m = np.ones((9, 12), dtype=np.int32)
    m[0, 0] = 0
    h = sr.heights_oracle(m, max_distance=4)
    assert h.max() == 16 and h[0, 1] == 0 and h[8, 11] == 16
    assert (sr.heights_oracle(np.ones((5, 7), dtype=np.int32)) == sr.FAR).all()          # no border inside the image: all far


# ---- insar_unet_ca_amd/split.py without a device -----------------------------------------------------------------------------
def test_exports_and_abi():
    import insar_unet_ca_amd as iu
    for name in ("split_regions", "SplitScratch"):
        assert name in iu.__all__ and hasattr(iu, name)
    assert iu.split_regions is sp.split_regions
    assert _lib.ABI_VERSION == 8 and _lib.load().insar_version() == 8
    for name in ("insar_split_scratch_bytes", "insar_split_basins", "insar_split_rounds", "insar_split_finish"):
        assert name in _lib.EXPORTED_SYMBOLS


def test_scratch_bytes_arithmetic():
    a16 = lambda b: (b + 15) // 16 * 16
    for H, W, mr, mp, rounds in ((1, 1, 1, 1, 1), (70, 150, 100, 1000, 64), (61, 131, 65536, 1 << 20, 64), (200, 1, 7, 8, 5)):
        s, t, off, cb = sp.scratch_bytes(H, W, mr, mp, rounds)
        seg, cap = a16(4 * H * W), 2
        while cap < 2 * mp:
            cap *= 2
        assert t == 80 * (mr + 1) and cb == a16(4 * (8 + rounds))
        assert off == 6 * seg + a16(4 * ((H * W + 1023) // 1024))
        assert s == off + cb + 16 * cap + 16 * mp
        assert off % 16 == 0 and s % 16 == 0
    assert sp.SPLIT_DTYPE.itemsize == 80 and sp.SPLIT_DTYPE.fields["first"][1] == 48 and sp.SPLIT_DTYPE.fields["saddle"][1] == 68
    for bad in ((0, 4, 1, 1, 1), (4, 4, 0, 1, 1), (4, 4, 1, 0, 1), (4, 4, 1, (1 << 24) + 1, 1), (4, 4, 1, 1, 0), (4, 4, 1, 1, 4097),
                (65536, 32768, 1, 1, 1)):
        with pytest.raises(InsarError):
            sp.scratch_bytes(*bad)


def test_entry_points_check_arguments_before_the_device():
    buf = (C.c_char * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_split_basins", None, p, 4, 4, 8, 4, p, None)
    with pytest.raises(InsarError, match="aligned"):
        _lib.call("insar_split_basins", p, p, 4, 4, 8, 4, p + 4, None)
    with pytest.raises(InsarError, match="threshold"):
        _lib.call("insar_split_rounds", p, 4, 4, 1, (1 << 20) + 1, 0, 1, 8, 4, p, None)
    with pytest.raises(InsarError, match="rounds"):
        _lib.call("insar_split_rounds", p, 4, 4, 1, 0, 3, 2, 8, 4, p, None)
    with pytest.raises(InsarError, match="max_regions"):
        _lib.call("insar_split_finish", p, p, None, None, 4, 4, 0, 8, 4, p, p, p, None)
    with pytest.raises(InsarError, match="max_pairs"):
        _lib.call("insar_split_finish", p, p, None, None, 4, 4, 1, 0, 4, p, p, p, None)


def test_split_regions_validates_without_a_gpu():
    lab = torch.zeros(8, 12, dtype=torch.int32)
    f = sp.split_regions
    with pytest.raises(InsarError, match="torch tensor"):
        f(np.zeros((8, 12), dtype=np.int32))
    for bad in (lab.long(), lab[None], lab.t()):
        with pytest.raises(InsarError, match="labels must be a contiguous 2-D int32"):
            f(bad)
    with pytest.raises(InsarError, match="mask must be a contiguous 2-D uint8"):
        f(lab, mask=lab)
    with pytest.raises(InsarError, match="mask .* for labels"):
        f(lab, mask=torch.zeros(8, 11, dtype=torch.uint8))
    with pytest.raises(InsarError, match="conf must be a contiguous 2-D float32"):
        f(lab, conf=lab.double())
    with pytest.raises(InsarError, match="height must be a contiguous 2-D int32"):
        f(lab, height=lab.float())
    with pytest.raises(InsarError, match="height .* for labels"):
        f(lab, height=torch.zeros(9, 12, dtype=torch.int32))
    with pytest.raises(InsarError, match="max_distance belongs"):
        f(lab, height=lab, max_distance=3)
    with pytest.raises(InsarError, match="squared"):
        f(lab, squared=1)
    for bad in (-1, float("nan"), "1", 1 << 17, True):
        with pytest.raises(InsarError, match="min_depth"):
            f(lab, min_depth=bad)
    with pytest.raises(InsarError, match="min_depth=1.5: an integer"):
        f(lab, height=lab, min_depth=1.5)
    for name, bad in (("max_distance", 0), ("max_distance", 40000), ("max_regions", 0), ("max_pairs", 0),
                      ("max_pairs", (1 << 24) + 1), ("max_rounds", 0), ("max_rounds", 4097), ("max_rounds", 2.5)):
        with pytest.raises(InsarError, match=name):
            f(lab, **{name: bad})
    with pytest.raises(InsarError, match="SplitScratch"):
        f(lab, scratch=object())
    with pytest.raises(InsarError, match="ROCm tensor"):                      # every other check comes first
        f(lab, mask=torch.zeros(8, 12, dtype=torch.uint8), conf=torch.zeros(8, 12), min_depth=2.0, max_distance=5)


def test_table_parsing_and_the_region_limit():
    raw = np.zeros(3, dtype=sp.SPLIT_DTYPE)
    raw["area"] = (2, 6, 3)
    raw["sum_y"][1:], raw["sum_x"][1:], raw["sum_conf"][1:] = (9, 3), (12, 30), (3 << 30, 3 << 29)
    raw["peak_index"][1:], raw["saddle"][1:], raw["parent"][1:], raw["peak"][1:], raw["cls"][1:] = (13, 25), (4, -1), (7, 7), (9, 5), (1, 2)
    t = sp.pieces_from_table(raw.view(np.uint8), 10, 2, True)
    assert t["id"].tolist() == [1, 2] and t["cy"].tolist() == [1.5, 1.0] and t["cx"].tolist() == [2.0, 10.0]
    assert t["mean_conf"].tolist() == [0.5, 0.5] and t["peak_y"].tolist() == [1, 2] and t["peak_x"].tolist() == [3, 5]
    assert t["saddle"].tolist() == [4, -1] and t["parent"].tolist() == [7, 7] and t["cls"].tolist() == [1, 2]
    assert "mean_conf" not in sp.pieces_from_table(raw.view(np.uint8), 10, 2, False)
    with pytest.raises(InsarError, match="max_regions=1"):
        sp.pieces_from_table(raw.view(np.uint8), 10, 1, False)
