"""CPU: the numpy restatement of the sieve (tests/sieve_ref.py) pinned on the prototype's findings, the `min_area` forms and
every argument refusal of insar_unet_ca_amd.sieve, none of which needs a device (devices are checked last)."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from insar_unet_ca_amd import sieve as sv
from insar_unet_ca_amd._lib import InsarError
from tests import sieve_ref as ref


def _cases():
    for H, W in ref.SHAPES:
        for conn in (4, 8):
            yield H, W, conn


@pytest.mark.parametrize("H,W,conn", list(_cases()))
def test_postcondition_and_idempotence(H, W, conn):
    m = ref.blob_speckle(H, W, seed=H * 1000 + W)
    T = {0: 9, 1: 14}
    res = ref.sieve(m, T, connectivity=conn)
    assert res["converged"] and ref.violations(res, T) == []
    assert np.array_equal(res["mask"] == 255, m == 255) and res["changed_pixels"] == int((res["mask"] != m).sum())
    again = ref.sieve(res["mask"], T, connectivity=conn)
    assert again["rounds"] == 0 and again["converged"] and again["absorbed"] == 0 and np.array_equal(again["mask"], res["mask"])


def test_labels_are_numbered_by_first_pixel_and_cover_class_zero():
    m = np.array([[0, 0, 1, 1], [2, 0, 1, 255], [2, 2, 0, 0]], dtype=np.uint8)
    labels, area, cls = ref.label_all(m, connectivity=4)
    assert labels.tolist() == [[1, 1, 2, 2], [3, 1, 2, 0], [3, 3, 4, 4]]
    assert area.tolist() == [0, 3, 3, 3, 2] and cls.tolist() == [0, 0, 1, 2, 0]
    labels8, _, _ = ref.label_all(m, connectivity=8)
    assert labels8.tolist() == [[1, 1, 2, 2], [3, 1, 2, 0], [3, 3, 1, 1]]
    none, _, cls_none = ref.label_all(m, connectivity=4, void_value=None)
    assert none[1, 3] == 4 and cls_none[4] == 255 and none.max() == 5


def test_adjacency_counts_shared_pixel_edges():
    labels = np.array([[1, 1, 2], [1, 3, 2], [0, 3, 3]], dtype=np.int32)
    adj = ref.adjacency(labels)
    assert list(zip(adj["a"], adj["b"], adj["edges"])) == [(1, 2, 1), (1, 3, 2), (2, 3, 2)] and adj["count"] == 3
    assert ref.adjacency(np.ones((4, 5), dtype=np.int32))["count"] == 0
    assert ref.adjacency(np.array([[7]], dtype=np.int32))["count"] == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_binary_map_equals_drop_small_components(seed):
    """Without void, and where every small region has a neighbour, {1: t} is label_regions(min_area=t)'s mask."""
    rng = np.random.default_rng(seed)
    m = (ndimage.uniform_filter(rng.random((40, 56)), 5) > 0.5).astype(np.uint8)
    m ^= (rng.random(m.shape) < 0.05).astype(np.uint8)
    t = 12
    res = ref.sieve(m, {1: t}, connectivity=8, void_value=None)
    lab, n = ndimage.label(m == 1, structure=np.ones((3, 3)))
    small = np.flatnonzero(np.bincount(lab.ravel(), minlength=n + 1) < t)
    want = np.where(np.isin(lab, small[small > 0]), 0, m).astype(np.uint8)
    assert np.array_equal(res["mask"], want) and res["absorbed"] == int((small > 0).sum()) > 0


def test_lone_region_stays():
    one = np.ones((1, 1), dtype=np.uint8)
    res = ref.sieve(one, {1: 5}, void_value=None)
    assert res["mask"].tolist() == [[1]] and res["rounds"] == 0 and res["converged"] and res["absorbed"] == 0
    boxed = np.full((5, 5), 255, dtype=np.uint8)                  # enclosed by void only: no neighbour
    boxed[2, 2] = 1
    assert np.array_equal(ref.sieve(boxed, 100)["mask"], boxed)


def test_class_zero_threshold_fills_exactly_the_small_holes():
    m = np.ones((20, 30), dtype=np.uint8)
    m[0, :] = 0                                                   # the outer background: 30 px
    m[4:6, 4:7] = 0                                               # a 6 px hole
    m[10:14, 10:14] = 0                                           # a 16 px hole
    m[16, 20] = 0                                                 # a pinhole
    res = ref.sieve(m, {0: 16}, connectivity=4)
    want = m.copy()
    want[4:6, 4:7] = 1
    want[16, 20] = 1
    assert np.array_equal(res["mask"], want) and res["absorbed"] == 2 and res["changed_pixels"] == 7 and res["rounds"] == 1


@pytest.mark.parametrize("case", [ref.STRIPS_2, ref.STRIPS_3], ids=["two_rounds", "three_rounds"])
def test_strip_maps_need_their_rounds(case):
    widths, t, rounds = case
    m = ref.strips(widths)
    res = ref.sieve(m, t, void_value=None)
    assert res["rounds"] == rounds and res["converged"] and ref.violations(res, t) == []
    assert (res["mask"] == 1).all()                               # everything ends in the long class-1 strip
    one = ref.sieve(m, t, void_value=None, max_rounds=1)
    assert one["rounds"] == 1 and one["converged"] is False
    exact = ref.sieve(m, t, void_value=None, max_rounds=rounds)   # the idle round was never run
    assert exact["rounds"] == rounds and exact["converged"] is False and np.array_equal(exact["mask"], res["mask"])


def test_ties_go_to_the_smaller_id():
    m = ref.strips([4, 1, 4])                                     # 0000 1 0000: two neighbours of equal area
    res = ref.sieve(m, {1: 2}, void_value=None)
    assert res["root"].tolist() == [0, 1, 1, 3]
    m = ref.strips([3, 3])                                        # a mutual pair of equal areas: the smaller id stays root
    res = ref.sieve(m, 5, void_value=None)
    assert res["root"].tolist() == [0, 1, 1] and (res["mask"] == 0).all() and res["rounds"] == 1
    m = ref.strips([2, 3])                                        # ... of different areas: the larger one stays
    assert (ref.sieve(m, 5, void_value=None)["mask"] == 1).all()


def test_min_area_forms_build_the_same_table():
    want = np.zeros(256, dtype=np.int32)
    want[0], want[1] = 16, 64
    for form in ({1: 64, 0: 16}, [16, 64], (16, 64), np.array([16, 64]), {np.int64(1): 64.0, 0: np.int32(16)}):
        T = sv.threshold_table(form)
        assert T.dtype == np.int32 and np.array_equal(T, want), form
        assert np.array_equal(ref.table(form), want)
    assert np.array_equal(sv.threshold_table(7), np.full(256, 7)) and np.array_equal(sv.threshold_table(7.0), ref.table(7))
    assert not sv.threshold_table({}).any() and not sv.threshold_table([]).any()


def test_scratch_bytes_is_host_arithmetic():
    total, off, cb, poff = sv.scratch_bytes(100, 130, 1000, 4096, 64)
    assert off == (100 * 130 + 15) // 16 * 16 and cb == (8 + 64) * 4 and poff % 16 == 0 and off + cb + 6 * 4 * 1001 <= poff
    assert total == poff + 16 + 16 * 4096 + 16 * 8192
    for bad in ((0, 5, 1, 1, 1), (1 << 16, 1 << 15, 1, 1, 1), (4, 4, 0, 1, 1), (4, 4, 1, 0, 1), (4, 4, 1, (1 << 24) + 1, 1),
                (4, 4, 1, 1, 0), (4, 4, 1, 1, 4097)):
        with pytest.raises(InsarError):
            sv.scratch_bytes(*bad)


def test_every_argument_error_is_raised_by_name():
    m = torch.zeros(6, 8, dtype=torch.uint8)
    bad = [
        (dict(mask=np.zeros((6, 8), np.uint8)), "mask must be a torch tensor"),
        (dict(mask=m.int()), "mask must be"),
        (dict(mask=m[None]), "mask must be"),
        (dict(mask=m.t()), "mask must be"),
        (dict(mask=torch.zeros(0, 8, dtype=torch.uint8)), "need H, W >= 1"),
        (dict(min_area="big"), "min_area='big'"),
        (dict(min_area=True), "min_area=True"),
        (dict(min_area=-1), "min_area=-1"),
        (dict(min_area=1.5), "min_area=1.5"),
        (dict(min_area={256: 3}), "min_area: class=256"),
        (dict(min_area={1: -2}), r"min_area\[1\]=-2"),
        (dict(min_area=[1, "x"]), r"min_area\[1\]='x'"),
        (dict(min_area=list(range(257))), "at most 256 entries"),
        (dict(connectivity=6), "connectivity=6"),
        (dict(void_value=256), "void_value=256"),
        (dict(void_value=1.0), "void_value=1.0"),
        (dict(max_regions=0), "max_regions=0"),
        (dict(max_pairs=(1 << 24) + 1), "max_pairs="),
        (dict(max_rounds=0), "max_rounds=0"),
        (dict(max_rounds=4097), "max_rounds=4097"),
        (dict(return_changed=1), "return_changed=1"),
        (dict(scratch=object()), "scratch must be a SieveScratch"),
        (dict(), "mask must be a ROCm tensor"),                   # the device comes last
    ]
    for kw, msg in bad:
        args = dict(mask=m, min_area=4)
        args.update(kw)
        mask = args.pop("mask")
        with pytest.raises(InsarError, match=msg):
            sv.sieve_regions(mask, **args)
    with pytest.raises(TypeError):
        sv.sieve_regions(m)                                       # min_area has no default

    lab = torch.zeros(6, 8, dtype=torch.int32)
    for args, kw, msg in [((m,), {}, "labels must be"), ((lab[None],), {}, "labels must be"),
                          ((lab,), dict(max_pairs=0), "max_pairs=0"), ((lab,), dict(scratch=3), "scratch must be a SieveScratch"),
                          ((lab,), {}, "labels must be a ROCm tensor")]:
        with pytest.raises(InsarError, match=msg):
            sv.region_adjacency(*args, **kw)


def test_exports():
    import insar_unet_ca_amd as iu
    assert iu.sieve_regions is sv.sieve_regions and iu.region_adjacency is sv.region_adjacency and iu.SieveScratch is sv.SieveScratch
