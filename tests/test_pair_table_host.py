"""CPU: the key counts of tests/pair_table_cases.py from the numpy oracles alone, so that tests/test_pair_table_gpu.py holds the
device table to numbers that do not come from it."""
import numpy as np
import pytest

from tests import pair_table_cases as cases
from tests import split_ref


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_every_pixel_carries_an_overlap_pair_of_its_own(H, W):
    pred, gt, (p, g, n) = cases.overlaps_case(H, W)
    assert len(p) == H * W > 16 and (n == 1).all()
    assert np.array_equal(np.sort(p), np.arange(1, H * W + 1)) and np.array_equal(p + g, np.full(H * W, H * W + 1))


@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_every_pixel_edge_is_an_adjacent_pair(H, W):
    labels, adj = cases.adjacency_case(H, W)
    assert adj["count"] == H * (W - 1) + W * (H - 1) > 16 and (adj["edges"] == 1).all()
    assert set((adj["b"] - adj["a"]).tolist()) == {1, W}


@pytest.mark.parametrize("H,W,P", [(8, 9, 52), (7, 10, 52), (8, 12, 65)])
def test_summits_on_the_even_lattice_are_the_basins(H, W, P):
    assert (H, W) in cases.SHAPES
    labels, height, pairs = cases.split_case(H, W)
    basin = split_ref.basins_oracle(labels, height)
    y, x = np.divmod(np.unique(basin), W)
    assert len(y) == ((H + 1) // 2) * ((W + 1) // 2) and (y % 2 == 0).all() and (x % 2 == 0).all()
    assert pairs == P > 16
    # nothing merges at depth 0: every saddle lies below both of its summits
    assert max(split_ref.saddles_oracle(labels, height, basin).values()) < 100 <= height.ravel()[np.unique(basin)].min()
