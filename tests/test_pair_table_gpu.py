"""GPU: the one pair table of csrc/pair_table.h held to its limits through each of its three users, region_overlaps
(csrc/overlap.hip, values added), region_adjacency (csrc/sieve.hip, values added) and split_regions (csrc/split.hip, values
raised to a maximum), on the maps of tests/pair_table_cases.py, whose key counts P tests/test_pair_table_host.py pins.

For every tool and shape: max_pairs = P gives exactly the oracle's result; max_pairs = P - 1 (a table of at least P slots, so
nothing is dropped) is refused with the true count P; max_pairs = 8 (16 slots for more than 16 keys) fills the table, takes the
overflow path and is refused in the tool's words for a full table. Every call here allocates its own scratch. That the clear
launch zeroes its second range on a scratch that is used again is held elsewhere: the output header of overlaps by
test_score_gpu.py::test_twenty_calls_are_byte_identical (table and output filled with 0xFF, then reused), the pair list's
header of sieve and the control words of split by test_reused_scratch_is_bitwise_reproducible of test_sieve_gpu.py and
test_split_gpu.py."""
import numpy as np
import pytest
import torch

from insar_unet_ca_amd._lib import InsarError
from tests import pair_table_cases as cases
from tests import sieve_ref, split_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _refused(call, P, pairs, full):
    """max_pairs = P - 1 names the true count and no full table; max_pairs = 8 names a full table (`full`)."""
    with pytest.raises(InsarError, match=rf"\b{P} {pairs} exceed max_pairs={P - 1}\b") as e:
        call(P - 1)
    assert "more than" not in str(e.value) and "full table" not in str(e.value)
    with pytest.raises(InsarError, match=rf"{full}.* exceed max_pairs=8\b") as e:
        call(8)
    assert pairs in str(e.value)


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_region_overlaps_at_its_limits(dev, H, W):
    import insar_unet_ca_amd as iu
    pred, gt, want = cases.overlaps_case(H, W)
    P = len(want[0])
    p, g = _t(pred, dev), _t(gt, dev)
    got = iu.region_overlaps(p, g, max_pairs=P)
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    _refused(lambda mp: iu.region_overlaps(p, g, max_pairs=mp), P, "overlapping pairs", "and a full table")


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_region_adjacency_at_its_limits(dev, H, W):
    import insar_unet_ca_amd as iu
    labels, want = cases.adjacency_case(H, W)
    P = want["count"]
    t = _t(labels, dev)
    got = iu.region_adjacency(t, max_pairs=P)
    assert got["count"] == P
    assert all(got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]) for f in ("a", "b", "edges"))
    _refused(lambda mp: iu.region_adjacency(t, max_pairs=mp), P, "adjacent region pairs", "more than")


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_sieve_regions_refuses_a_full_pair_table(dev, H, W):
    """The same table behind sieve_regions: a class map whose regions are single pixels (a checkerboard of two classes under
    4-connectivity) has the pairs of `adjacency_case`."""
    import insar_unet_ca_amd as iu
    y, x = np.mgrid[0:H, 0:W]
    board = ((y + x) % 2).astype(np.uint8)
    P = H * (W - 1) + W * (H - 1)
    assert sieve_ref.adjacency(sieve_ref.label_all(board, 4)[0])["count"] == P
    m = _t(board, dev)
    out = iu.sieve_regions(m, min_area=0, connectivity=4, max_regions=H * W, max_pairs=P)
    assert out["regions_in"] == H * W and out["absorbed"] == 0 and torch.equal(out["mask"], m)
    _refused(lambda mp: iu.sieve_regions(m, min_area=0, connectivity=4, max_regions=H * W, max_pairs=mp), P,
             "adjacent region pairs", "more than")


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_split_regions_at_its_limits(dev, H, W):
    import insar_unet_ca_amd as iu
    labels, height, P = cases.split_case(H, W)
    want = split_ref.split_oracle(labels, height=height, squared=False, min_depth=0)
    l, h = _t(labels, dev), _t(height, dev)
    run = lambda mp: iu.split_regions(l, height=h, squared=False, min_depth=0, max_pairs=mp)
    got = run(P)
    assert (got["raw_basins"], got["count"], got["rounds"], got["converged"]) == \
           (want["raw_basins"], want["count"], want["rounds"], want["converged"])
    assert np.array_equal(got["labels"].cpu().numpy(), want["labels"])
    # the saddle of a piece is the maximum that the table keeps per pair, taken over the piece's pairs
    for f in ("area", "peak", "peak_y", "peak_x", "saddle", "parent"):
        assert np.array_equal(got["regions"][f], want["regions"][f]), f
    _refused(run, P, "adjacent basin pairs", "more than")
