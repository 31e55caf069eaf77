"""CPU-only: the centre-line oracle (tests/skeleton_ref.py) against its invariants and hand-made shapes, the host conversion
`skeleton_table`, the record layout against the C compiler, the host-only queries and every argument check of
insar_unet_ca_amd/skeletons.py that needs no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

from insar_unet_ca_amd import _lib
from insar_unet_ca_amd import skeletons as sk
from insar_unet_ca_amd._lib import InsarError
from tests import skeleton_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insar_hip.h")
EIGHT = np.ones((3, 3), dtype=int)


def _maps():
    """(name, labels int32): 96 x 130 blobs and 64 x 64 speckle, labelled with 4- and 8-connectivity."""
    out = []
    for seed in (1, 2):
        for c in (4, 8):
            out.append((f"blobs {seed} conn {c}", ref.label_scipy(ref.blobs(96, 130, seed), c)))
    for c in (4, 8):
        out.append((f"speckle conn {c}", ref.label_scipy(ref.speckle(64, 64, 5), c)))
    return out


MAPS = _maps()


@pytest.mark.parametrize("name,labels", MAPS, ids=[m[0] for m in MAPS])
def test_oracle_invariants(name, labels):
    alive, iterations, converged = ref.thin_oracle(labels, 64)
    assert converged and iterations <= 16, (name, iterations)
    assert not (alive & (labels <= 0)).any()                                  # a subset of the regions
    again = ref.thin_oracle(np.where(alive, labels, 0), 64)
    assert again[1] == 0 and (again[0] == alive).all()                        # idempotent
    n_lab = int(labels.max())
    assert n_lab > 3
    alone = np.zeros_like(alive)
    for l in range(1, n_lab + 1):
        region = labels == l
        s = alive & region
        assert s.any(), (name, l)
        assert ndimage.label(s, structure=EIGHT)[1] == 1, (name, l)           # one 8-connected piece
        holes = lambda m: ndimage.label(~np.pad(m, 1))[1]                     # 4-connected background components
        assert holes(s) == holes(region), (name, l)
        alone |= ref.thin_oracle(region.astype(np.int32), 64)[0]
    assert (alone == alive).all()                                             # per region = each region alone


def test_hand_cases():
    got = {k: ref.skeleton_oracle(m, 40) for k, m in ref.HAND.items()}
    for k, it in ref.HAND_ITERATIONS.items():
        assert got[k]["iterations"] == it and got[k]["converged"], k
    bar = got["bar 3x9"]["skeleton"]
    assert (np.argwhere(bar > 0) == [[3, x] for x in range(3, 10)]).all()     # the middle row without its two end pixels
    assert bar[3, 3:10].tolist() == [2, 3, 3, 3, 3, 3, 2]
    for k in ("block 2x2", "block 5x5", "full 8x8", "square 70x70"):
        assert (got[k]["skeleton"] > 0).sum() == 1 and got[k]["skeleton"].max() == 1, k
    ring = got["ring 9x9"]["skeleton"]
    assert (ring > 0).sum() == 18 and set(ring[ring > 0].tolist()) == {3}
    assert ndimage.label(ring == 0)[1] == 2                                   # closed: the hole stays cut off
    st = got["ring 9x9"]["stats"]
    assert st["n"].tolist() == [18] and st["n_orth"][0] + st["n_diag"][0] == 18 and st["n_end"].tolist() == [0]
    assert got["full 8x8"]["stats"]["n_far"].tolist() == [1]                  # a region that fills the image has no edge site
    long = got["bar 9x200"]["stats"]
    assert long["n_end"].tolist() == [2] and long["n_orth"][0] == long["n"][0] - 1 and long["max_d2"].tolist() == [16]


def test_bound_cuts_short():
    m = ref.HAND["square 70x70"]
    full = ref.thin_oracle(m, 40)[0]
    for mi in (1, 2, 3, 9, 34):
        alive, it, conv = ref.thin_oracle(m, mi)
        assert it == mi and not conv and alive.sum() > full.sum()
    last = ref.thin_oracle(m, 35)
    assert last[1] == 35 and not last[2] and (last[0] == full).all()          # finished by the last one allowed: conservative
    assert ref.thin_oracle(m, 36)[2]


# ---- host conversion --------------------------------------------------------------------------------------------------------
def _records(pixels, d2=None, far=()):
    """Hand-made accumulators of one region from a pixel list [(y, x), ...] in skeleton order (consecutive ones are linked)."""
    r = np.zeros(1, dtype=sk.STAT_DTYPE)
    ys, xs = np.array([p[0] for p in pixels]), np.array([p[1] for p in pixels])
    r["n"], r["sum_y"], r["sum_x"] = len(pixels), ys.sum(), xs.sum()
    r["sum_yy"], r["sum_xx"], r["sum_xy"] = (ys * ys).sum(), (xs * xs).sum(), (ys * xs).sum()
    for a, b in zip(pixels[:-1], pixels[1:]):
        r["n_orth" if abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 else "n_diag"] += 1
    r["n_end"] = 2 if len(pixels) > 1 else 0
    if d2 is not None:
        keep = [v for i, v in enumerate(d2) if i not in far]
        r["sum_d2"], r["max_d2"], r["n_far"] = sum(keep), max(keep, default=0), len(far)
    return r


def test_table_lines():
    n = 9
    t = sk.skeleton_table(_records([(5, 3 + i) for i in range(n)], d2=[4] * n))
    assert t["orientation"][0] == 0.0 and t["length"][0] == n - 1 and np.isinf(t["elongation"][0])
    assert t["mean_width"][0] == 5.0 and t["max_width"][0] == 5.0 and t["n_end"][0] == 2 and t["label"].tolist() == [1]
    t = sk.skeleton_table(_records([(3 + i, 7) for i in range(n)]))
    assert t["orientation"][0] == pytest.approx(90.0, abs=1e-12) and t["length"][0] == n - 1
    t = sk.skeleton_table(_records([(2 + i, 4 + i) for i in range(n)]))       # top left to bottom right: 45 by the convention
    assert t["orientation"][0] == pytest.approx(45.0, abs=1e-12) and t["length"][0] == pytest.approx((n - 1) * np.sqrt(2), rel=1e-15)
    t = sk.skeleton_table(_records([(12 - i, 4 + i) for i in range(n)]))      # bottom left to top right
    assert t["orientation"][0] == pytest.approx(135.0, abs=1e-12)


def test_table_degenerate_records():
    one = sk.skeleton_table(_records([(4, 4)], d2=[9]))
    assert np.isnan(one["orientation"][0]) and np.isnan(one["elongation"][0]) and one["length"][0] == 0 and one["mean_width"][0] == 7.0
    far = sk.skeleton_table(_records([(4, 4), (4, 5)], d2=[sk._lib.DIST_FAR] * 2, far=(0, 1)))
    assert np.isnan(far["mean_width"][0]) and far["orientation"][0] == 0.0
    part = sk.skeleton_table(_records([(4, 4), (4, 5), (4, 6)], d2=[1, 4, 0], far=(2,)))
    assert part["mean_width"][0] == pytest.approx(2 * np.sqrt(2.5) + 1, rel=1e-15)
    empty = sk.skeleton_table(np.zeros(2, dtype=sk.STAT_DTYPE))
    assert np.isnan(empty["orientation"]).all() and (empty["length"] == 0).all() and empty["label"].tolist() == [1, 2]
    off = sk.skeleton_table(_records([(4, 4), (4, 5)]), widths=False)
    assert np.isnan(off["mean_width"][0]) and np.isnan(off["max_width"][0])


@pytest.mark.parametrize("name,labels", MAPS[:2] + MAPS[4:5], ids=[m[0] for m in MAPS[:2] + MAPS[4:5]])
def test_table_equals_the_oracles_formulas(name, labels):
    st = ref.skeleton_oracle(labels, 32)["stats"]
    got, want = sk.skeleton_table(st), ref.table_oracle(st)
    for f, v in want.items():
        np.testing.assert_allclose(got[f], v, rtol=1e-12, atol=0, equal_nan=True, err_msg=f)
    assert (got["n_end"] == st["n_end"]).all() and (got["n_junction"] == st["n_junction"]).all()
    assert (got["length"] >= 0).all() and ((got["orientation"] >= 0) & (got["orientation"] < 180) | np.isnan(got["orientation"])).all()


# ---- without a device -------------------------------------------------------------------------------------------------------
def test_stat_dtype_matches_the_c_compiler(tmp_path):
    fields = [f for f in sk.STAT_DTYPE.names]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(InsarSkeletonStat));']
    lines += [f'printf("{f} %zu\\n", offsetof(InsarSkeletonStat, {f}));' for f in fields]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == sk.STAT_DTYPE.itemsize == 80
    for f in fields:
        assert int(got[f]) == sk.STAT_DTYPE.fields[f][1], f


def test_queries():
    T = sk.ITERATIONS_PER_LAUNCH
    assert sk.launches(64, 64, 32, True) == 2 + 32 // T + 2 and sk.launches(64, 64, 32, False) == 2 + 32 // T
    assert sk.launches(1, 1, 1, False) == 3 and sk.launches(4096, 4096, T, False) == 3 and sk.launches(9, 9, T + 1, False) == 4
    assert sk.launches(32767, 32767, 32768, True) == 4 + 32768 // T          # a function of max_iterations and widths alone
    s, t = sk.scratch_bytes(64, 64, 32, 100)
    assert t == 80 * 101 and s % 16 == 0
    words = lambda H, W: H * ((W + 63) // 64)
    assert s >= 10 * 8 * words(64, 64) + 4 * 32
    # monotone in every argument, and ten planes of one word per 64 pixels of a row carry most of it
    assert sk.scratch_bytes(65, 64, 32, 100)[0] > s and sk.scratch_bytes(64, 65, 32, 100)[0] > s and sk.scratch_bytes(64, 64, 64, 100)[0] > s
    big, _ = sk.scratch_bytes(4096, 4096, 32)
    assert 10 * 8 * words(4096, 4096) <= big <= 10 * 8 * words(4096, 4096) + (1 << 16)
    for bad in ((0, 5, 32, 1), (5, 32768, 32, 1), (5, 5, 0, 1), (5, 5, 32769, 1), (5, 5, 32, 0)):
        with pytest.raises(InsarError):
            sk.scratch_bytes(*bad)
    with pytest.raises(InsarError, match="max_iterations"):
        sk.launches(5, 5, 0)


def test_c_argument_checks_without_a_device():
    call = _lib.call
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 15) & ~15
    with pytest.raises(InsarError, match="null"):
        call("insar_skeleton_planes", None, 8, 8, 32, 4, p, p, None)
    with pytest.raises(InsarError, match="null"):
        call("insar_skeleton_planes", p, 8, 8, 32, 4, p, None, None)
    with pytest.raises(InsarError, match="aligned"):
        call("insar_skeleton_planes", p, 8, 8, 32, 4, p + 8, p, None)
    with pytest.raises(InsarError, match="H and W"):
        call("insar_skeleton_planes", p, 8, 40000, 32, 4, p, p, None)
    with pytest.raises(InsarError, match="max_regions"):
        call("insar_skeleton_planes", p, 8, 8, 32, 0, p, p, None)
    with pytest.raises(InsarError, match="step 4 outside 0..3"):
        call("insar_skeleton_step", 8, 8, 32, 4, p, None)
    with pytest.raises(InsarError, match="step -1"):
        call("insar_skeleton_step", 8, 8, 32, -1, p, None)
    with pytest.raises(InsarError, match="null"):
        call("insar_skeleton_step", 8, 8, 32, 0, None, None)
    with pytest.raises(InsarError, match="null pointer \\(skeleton\\)"):
        call("insar_skeleton_stats", p, None, 8, 8, 32, 4, p, p, None, None)
    with pytest.raises(InsarError, match="max_iterations"):
        call("insar_skeleton_stats", p, None, 8, 8, 0, 4, p, p, p, None)
    with pytest.raises(InsarError, match="aligned"):
        call("insar_skeleton_stats", p, p + 2, 8, 8, 32, 4, p, p, p, None)


def test_python_argument_checks_without_a_device():
    good = torch.zeros(8, 8, dtype=torch.int32)
    cases = [(dict(labels=np.zeros((8, 8), np.int32)), "torch tensor"), (dict(labels=good.long()), "int32"),
             (dict(labels=good[None]), "2-D"), (dict(labels=good.t()[:, ::2]), "contiguous"),
             (dict(labels=torch.zeros(0, 8, dtype=torch.int32)), "H, W"), (dict(max_iterations=0), "max_iterations"),
             (dict(max_iterations=1.5), "max_iterations"), (dict(max_iterations=True), "max_iterations"),
             (dict(max_iterations=40000), "max_iterations"), (dict(widths=1), "widths"), (dict(max_regions=0), "max_regions"),
             (dict(max_regions=2.0), "max_regions"), (dict(scratch=object()), "SkeletonScratch")]
    for kw, what in cases:
        kw = dict({"labels": good}, **kw)
        with pytest.raises(InsarError, match=what):
            sk.thin_regions(kw.pop("labels"), **kw)
    with pytest.raises(InsarError, match="ROCm tensor"):                      # the device is checked last
        sk.thin_regions(good)
    import insar_unet_ca_amd as iu
    assert iu.thin_regions is sk.thin_regions and iu.SkeletonScratch is sk.SkeletonScratch and iu.skeleton_table is sk.skeleton_table
