"""The maps of tests/test_pair_table_gpu.py (a helper, not a test module): tiny scenes that put as many keys as possible into
the pair table of csrc/pair_table.h through each of its three users, with the key count P from the tools' numpy oracles.
tests/test_pair_table_host.py pins the counts on the CPU.

8 x 9 and 7 x 10 are off the width of a 16-byte access (W % 4 != 0; 70 pixels are no whole number of quads either), 8 x 12 is
on it. P > 16 everywhere: max_pairs = 8 gives a table of 16 slots, which fills up."""
import numpy as np

from tests import sieve_ref, split_ref
from tests.score_ref import overlaps_oracle

SHAPES = [(8, 9), (7, 10), (8, 12)]


def pixel_ids(H, W):
    """Every pixel its own region: ids 1..H W in row-major order."""
    return np.arange(1, H * W + 1, dtype=np.int32).reshape(H, W)


def overlaps_case(H, W):
    """(pred, gt, oracle table): every pixel its own region on both sides, numbered from opposite corners, so every pixel
    carries a pair of its own: P = H W."""
    pred = pixel_ids(H, W)
    gt = np.ascontiguousarray(pred[::-1, ::-1])
    return pred, gt, overlaps_oracle(pred, gt)


def adjacency_case(H, W):
    """(labels, oracle table): every pixel its own region, so every pixel edge is a pair: P = H (W - 1) + W (H - 1)."""
    labels = pixel_ids(H, W)
    return labels, sieve_ref.adjacency(labels)


def split_case(H, W):
    """(labels, height, P): one label over the whole map and a summit on every pixel with even y and even x, so every other
    pixel has a summit among its 8 neighbours: ceil(H / 2) ceil(W / 2) basins of at most 3 x 3 pixels, the most a height map
    can give (of two adjacent pixels of one label only one is a root). The ground between the summits varies, so the saddles
    of a pair differ from pixel to pixel. P counts the pairs of basins with 8-adjacent pixels."""
    labels = np.ones((H, W), dtype=np.int32)
    y, x = np.mgrid[0:H, 0:W]
    height = np.where((y % 2 == 0) & (x % 2 == 0), 100 + (3 * y + 5 * x) % 11, (7 * y + 3 * x) % 13).astype(np.int32)
    basin = split_ref.basins_oracle(labels, height)
    return labels, height, len(split_ref.saddles_oracle(labels, height, basin))
