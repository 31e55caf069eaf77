"""CPU-only: the oracles of tests/distance_ref.py pinned against an all-pairs brute force and scipy's exact EDT, boundary IoU
by hand, and the argument validation of insar_unet_ca_amd/distance.py and of its C entry points (no device is touched)."""
import ctypes as C

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _lib, distance
from insar_unet_ca_amd._lib import InsarError
from tests.distance_ref import (FAR, boundary_counts_oracle, brute_oracle, cap, dist_oracle, expand_labels_oracle,
                                nearest_oracle, sites_oracle, void_band_oracle)


def random_sites(H, W, fill, seed):
    s = np.random.default_rng(seed).random((H, W)) < fill
    s[H // 2, W // 3] = True                                          # never empty
    return s


# ---- the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0.002, 0.05, 0.5])
def test_separable_oracle_equals_all_pairs(fill):
    site = random_sites(40, 56, fill, seed=int(fill * 1000))
    d2, near = brute_oracle(site)
    assert (dist_oracle(site) == d2).all()
    # the nearest site is a site, lies at the distance claimed, and no site with a smaller index is as near
    ny, nx = near // 56, near % 56
    yy, xx = np.indices(site.shape)
    assert site[ny, nx].all() and ((yy - ny) ** 2 + (xx - nx) ** 2 == d2).all()
    sy, sx = np.nonzero(site)
    for y, x in ((0, 0), (39, 55), (17, 23)):
        d = (y - sy) ** 2 + (x - sx) ** 2
        assert near[y, x] == (sy * 56 + sx)[d == d.min()].min()


@pytest.mark.parametrize("shape, fill", [((70, 130), 0.01), ((40, 56), 0.3)])
def test_oracle_equals_scipy_exact_edt(shape, fill):
    ndimage = pytest.importorskip("scipy.ndimage")
    site = random_sites(*shape, fill, seed=3)
    want = np.rint(ndimage.distance_transform_edt(~site) ** 2).astype(np.int64)
    assert (dist_oracle(site) == want).all()


def test_oracle_without_sites_and_cap():
    site = np.zeros((5, 7), dtype=bool)
    d2, near = nearest_oracle(site)
    assert (d2 == FAR).all() and (near == -1).all() and (cap(dist_oracle(site), None) == FAR).all()
    site[0, 0] = True
    d2, near = nearest_oracle(site, max_distance=5)
    assert d2[3, 4] == 25 and near[3, 4] == 0 and d2[4, 4] == FAR and near[4, 4] == -1 and d2[0, 5] == 25 and d2[0, 6] == FAR


def test_site_predicates():
    m = np.array([[1, 1, 2, 2],
                  [1, 1, 2, 255],
                  [1, 1, 255, 3]], dtype=np.uint8)
    assert (sites_oracle(m, ("eq", 2)) == (m == 2)).all() and (sites_oracle(m, ("ne", 1)) == (m != 1)).all()
    e = sites_oracle(m, "edge", None)
    assert e.tolist() == [[False, True, True, True], [False, True, True, True], [False, True, True, True]]
    e = sites_oracle(m, "edge", 255)                                  # void pixels are no sites and make none
    assert e.tolist() == [[False, True, True, False], [False, True, True, False], [False, False, False, False]]
    assert not sites_oracle(np.full((4, 4), 7, dtype=np.int32), "edge", None).any()          # the image border is no border


def test_consumer_oracles_by_hand():
    m = np.zeros((9, 9), dtype=np.uint8)
    m[:, 5:] = 1
    m[0, 0] = 255
    band = void_band_oracle(m, 1)
    assert (band[:, 3:7] == 255).all() and (band[1:, :3] == 0).all() and (band[:, 7:] == 1).all() and band[0, 0] == 255
    assert (void_band_oracle(m, 0)[:, 4:6] == 255).all() and (void_band_oracle(m, 0)[:, 3] == 0).all()
    lab = np.zeros((5, 12), dtype=np.int32)
    lab[2, 2], lab[2, 7] = 4, 9                                       # 5 apart = 2 * 2 + 1
    g = expand_labels_oracle(lab, 2)
    assert g[2].tolist() == [4, 4, 4, 4, 4, 9, 9, 9, 9, 9, 0, 0] and g[0, 2] == 4 and g[0, 3] == 0
    assert (expand_labels_oracle(lab, 0) == lab).all()
    g = expand_labels_oracle(lab, 3)                                  # x = 4, 5: 2 / 3 and 3 / 2 away; no tie, no merge
    assert g[2].tolist() == [4, 4, 4, 4, 4, 9, 9, 9, 9, 9, 9, 0]


# ---- boundary IoU -----------------------------------------------------------------------------------------------------------
def squares(H, W, boxes):
    m = np.zeros((H, W), dtype=np.uint8)
    for c, y, x, s in boxes:
        m[y:y + s, x:x + s] = c
    return m


def test_boundary_iou_by_hand():
    a = squares(40, 60, [(1, 5, 5, 12), (2, 20, 30, 10)])
    same = iu.boundary_iou(boundary_counts_oracle(a, a, 2, 4))
    assert same["iou"][:3].tolist() == [1.0, 1.0, 1.0] and np.isnan(same["iou"][3]) and same["mean_iou"] == 1.0
    # disjoint squares of class 1 farther apart than 2 d: no common band pixel; class 3 is in neither map
    b = squares(40, 60, [(1, 5, 40, 12), (2, 20, 30, 10)])
    c = boundary_counts_oracle(a, b, 2, 4)
    r = iu.boundary_iou(c)
    assert c[1, 0] == 0 and c[1, 1] > 0 and c[1, 2] > 0 and r["iou"][1] == 0.0 and np.isnan(r["iou"][3])
    assert r["iou"][2] > 0 and r["mean_iou"] == pytest.approx((0.0 + r["iou"][2]) / 2, rel=1e-15)
    # a ring of width 2 inside a 12-square: 12^2 - 8^2 pixels of class 1 within distance 1 of its border (d2 <= 1)
    assert boundary_counts_oracle(a, a, 1, 4)[1].tolist() == [144 - 64] * 3
    # void pixels leave all three counts, and make no border in gt
    v = a.copy()
    v[5:17, 0:5] = 255                                                # the background left of the class-1 square
    cv = boundary_counts_oracle(a, v, 1, 4)
    # pred keeps its whole ring; in gt the square's left side is no border: columns 5, 6 of rows 7..14 leave G_1
    assert cv[1].tolist() == [80 - 16, 80, 80 - 16]
    assert cv[0, 1] == boundary_counts_oracle(a, a, 1, 4)[0, 1] - 24  # columns 3, 4 of rows 5..16 are void: they leave P_0
    assert (cv[:, 0] <= np.minimum(cv[:, 1], cv[:, 2])).all()
    # counts of several scenes add
    both = iu.boundary_iou(c + cv)
    assert both["iou"][1] == (c[1, 0] + cv[1, 0]) / (c[1, 1] + cv[1, 1] + c[1, 2] + cv[1, 2] - c[1, 0] - cv[1, 0])
    none = iu.boundary_iou(np.zeros((3, 3), dtype=np.int64))
    assert np.isnan(none["iou"]).all() and np.isnan(none["mean_iou"])
    for bad in (np.zeros((3, 2), dtype=np.int64), np.zeros((1, 3), dtype=np.int64), np.zeros((3, 3)), -np.ones((2, 3), dtype=np.int64)):
        with pytest.raises(InsarError, match="counts"):
            iu.boundary_iou(bad)


def test_detection_score_accumulates_boundary_counts():
    base = {"num_classes": 3, "iou_threshold": 0.5,
            "per_class": {k: np.zeros(3, dtype=np.int64) for k in ("tp", "fp", "fn")} | {"iou_sum": np.zeros(3)}}
    acc = iu.DetectionScore(3)
    acc.update(base)
    assert "boundary" not in acc.compute() and set(acc.compute()) == {"per_class", "overall", "scenes"}
    c1, c2 = np.array([[9, 9, 9], [1, 4, 2], [0, 0, 0]]), np.array([[5, 6, 7], [2, 2, 3], [0, 1, 0]])
    for c in (c1, c2):
        acc.update(dict(base, boundary={"distance": 3, "counts": c, **iu.boundary_iou(c)}))
    got = acc.compute()
    assert got["scenes"] == 3 and got["boundary"]["scenes"] == 2 and got["boundary"]["distance"] == 3
    assert (got["boundary"]["counts"] == c1 + c2).all() and got["boundary"]["iou"][1] == 3 / (6 + 5 - 3)
    with pytest.raises(InsarError, match="distance"):
        acc.update(dict(base, boundary={"distance": 5, "counts": c1}))
    acc.reset()
    assert "boundary" not in acc.compute()


# ---- argument validation without a device ---------------------------------------------------------------------------------------
def test_python_arguments_are_refused_before_any_launch():
    u8 = torch.zeros(8, 9, dtype=torch.uint8)
    i32 = torch.zeros(8, 9, dtype=torch.int32)
    dt = iu.distance_transform
    with pytest.raises(InsarError, match="m must be uint8 or int32"):
        dt(torch.zeros(8, 9))
    with pytest.raises(InsarError, match="m must be a torch tensor"):
        dt(np.zeros((8, 9), dtype=np.uint8))
    for bad in (torch.zeros(9, dtype=torch.uint8), torch.zeros(1, 1, 8, 9, dtype=torch.uint8)):
        with pytest.raises(InsarError, match=r"m must be 2-D \[H, W\] or 3-D"):
            dt(bad)
    with pytest.raises(InsarError, match="m must be contiguous"):
        dt(u8.t())
    with pytest.raises(InsarError, match=r"m \(32768, 1\): need"):
        dt(torch.zeros(32768, 1, dtype=torch.uint8))
    with pytest.raises(InsarError, match=r"m \(1, 32768\): need"):
        dt(torch.zeros(1, 32768, dtype=torch.uint8))
    with pytest.raises(InsarError, match=r"m \(0, 4\): need"):
        dt(torch.zeros(0, 4, dtype=torch.uint8))
    for bad in ("edges", ("eq",), ("gt", 1), ("eq", 1.5), ("ne", None), 3):
        with pytest.raises(InsarError, match="sites"):
            dt(u8, sites=bad)
    for bad in (0, -1, 2.5, "3"):
        with pytest.raises(InsarError, match="max_distance"):
            dt(u8, max_distance=bad)
    with pytest.raises(InsarError, match="ignore_value"):
        dt(u8, ignore_value=-2)
    sc = iu.DistanceScratch(1, 8, 8, "cpu")
    assert (sc.B, sc.H, sc.W) == (1, 8, 8) and sc.scratch.numel() == distance.scratch_bytes(1, 8, 8)
    with pytest.raises(InsarError, match="scratch of 1 x 8 x 8"):
        dt(u8, scratch=sc)
    with pytest.raises(InsarError, match="scratch must be a DistanceScratch"):
        dt(u8, scratch=object())
    with pytest.raises(InsarError, match="m must be a ROCm tensor"):            # everything else in order: only the device is wrong
        dt(u8, sites=("eq", 1), max_distance=None, scratch=iu.DistanceScratch(1, 8, 9, "cpu"))

    with pytest.raises(InsarError, match="width"):
        iu.void_band(u8, -1)
    with pytest.raises(InsarError, match="mask must be uint8"):
        iu.void_band(i32, 2)
    with pytest.raises(InsarError, match="void_value"):
        iu.void_band(u8, 2, void_value=256)
    with pytest.raises(InsarError, match="labels must be int32"):
        iu.expand_labels(u8, 2)
    with pytest.raises(InsarError, match="distance"):
        iu.expand_labels(i32, -3)
    for k in (1, 9, 2.5):
        with pytest.raises(InsarError, match="num_classes"):
            iu.boundary_counts(u8, u8, 3, k)
    with pytest.raises(InsarError, match="distance"):
        iu.boundary_counts(u8, u8, -1, 2)
    with pytest.raises(InsarError, match="one shape"):
        iu.boundary_counts(u8, torch.zeros(9, 8, dtype=torch.uint8), 3, 2)
    with pytest.raises(InsarError, match="gt must be uint8"):
        iu.boundary_counts(u8, i32, 3, 2)
    with pytest.raises(InsarError, match="scratch of 1 x 8 x 8"):
        iu.boundary_counts(u8, u8, 3, 2, scratch=sc)
    with pytest.raises(InsarError, match="pred must be a ROCm tensor"):
        iu.boundary_counts(u8, u8, 3, 2)


def test_c_entry_points_validate_before_the_device():
    lib = _lib.load()
    buf = (C.c_int64 * 64)()                                          # 16-byte-aligned enough for the checks that come first
    p = C.addressof(buf)
    U8, EDGE = _lib.DIST_U8, _lib.DIST_EDGE
    t = lambda *a: lib.insar_dist_transform(*a)
    assert t(None, U8, 1, 8, 8, EDGE, -1, 4, p, p, None, None) == -1005 and b"null" in lib.insar_last_error()
    assert t(p, U8, 1, 8, 8, EDGE, -1, 4, None, p, None, None) == -1005 and b"scratch" in lib.insar_last_error()
    assert t(p, U8, 1, 8, 8, EDGE, -1, 4, p, None, None, None) == -1005 and b"d2" in lib.insar_last_error()
    assert t(p, 2, 1, 8, 8, EDGE, -1, 4, p, p, None, None) == -1002
    assert t(p, U8, 1, 8, 8, 3, -1, 4, p, p, None, None) == -1005 and b"site mode" in lib.insar_last_error()
    assert t(p, U8, 0, 8, 8, EDGE, -1, 4, p, p, None, None) == -1001
    assert t(p, U8, 1, 32768, 8, EDGE, -1, 4, p, p, None, None) == -1001
    assert t(p, U8, 1, 8, 32768, EDGE, -1, 4, p, p, None, None) == -1001
    assert t(p, U8, 3, 32767, 32767, EDGE, -1, 4, p, p, None, None) == -1001 and b"2^31" in lib.insar_last_error()
    assert t(p, U8, 1, 8, 8, EDGE, -1, 4, p, p + 2, None, None) == -1003
    c = lambda *a: lib.insar_dist_boundary_counts(*a)
    for i in range(4):
        args = [p, p, p, p]
        args[i] = None
        assert c(*args, 8, 8, 9, 2, 255, p, None) == -1005
    assert c(p, p, p, p, 8, 8, 9, 2, 255, None, None) == -1005
    assert c(p, p, p, p, 8, 8, 9, 1, 255, p, None) == -1001 and c(p, p, p, p, 8, 8, 9, 9, 255, p, None) == -1001
    assert c(p, p, p, p, 8, 8, -1, 2, 255, p, None) == -1005 and c(p, p, p, p, 8, 8, 9, 2, 256, p, None) == -1005
    assert c(p, p, p, p, 0, 8, 9, 2, 255, p, None) == -1001
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_dist_scratch_bytes", 1, 8, 8, None)


def test_scratch_bytes_are_monotone_and_aligned():
    sb = distance.scratch_bytes
    assert sb(1, 1, 1) == 16 and sb(1, 200, 264) >= 2 * 200 * 264
    prev = 0
    for B, H, W in ((1, 1, 1), (1, 3, 5), (1, 200, 264), (2, 200, 264), (2, 201, 264), (2, 201, 265), (1, 32767, 32767)):
        b = sb(B, H, W)
        assert b % 16 == 0 and b >= prev and b >= 2 * B * H * W
        prev = b
    for bad in ((0, 4, 4), (1, 32768, 4), (1, 4, 32768), (3, 32767, 32767)):
        with pytest.raises(InsarError, match="insar_dist_scratch_bytes"):
            sb(*bad)


def test_abi_is_additive():
    assert _lib.ABI_VERSION == 8 and _lib.load().insar_version() == 8
    for name in ("insar_dist_scratch_bytes", "insar_dist_transform", "insar_dist_boundary_counts"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert _lib.DIST_FAR == FAR == distance.FAR == 2 ** 31 - 1
    for name in ("DistanceScratch", "distance_transform", "void_band", "expand_labels", "boundary_counts", "boundary_iou"):
        assert name in iu.__all__ and hasattr(iu, name)
