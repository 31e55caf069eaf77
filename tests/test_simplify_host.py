"""CPU-only: the oracle of the outline simplification (tests/simplify_ref.py) pinned by invariants on rings from
tests/outlines_ref.outlines_oracle, the argument checks of `simplify_outlines` that fire before the device is touched, the
host queries, and `to_polygons(drop_collapsed=...)`."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _lib
from insar_unet_ca_amd import simplify as sm
from insar_unet_ca_amd._lib import InsarError
from tests import rasterise_ref as rr
from tests import simplify_ref as sr
from tests.outlines_ref import outlines_oracle

TOLERANCES = (0, 0.5, 1, 2.5, 8)
ROUNDS = 2048
MAPS = {"spiral": (sr.spiral(24), 8), "disc": (sr.disc(20, 48), 8), "ring_island": (sr.ring_with_island(), 8),
        "staircase": (sr.two_label_staircase(), 8), "three_labels": (sr.three_labels(), 8), "three_labels4": (sr.three_labels(), 4),
        "blobs": (sr.blobs(40, 56, seed=9), 8), "checkerboard": (sr.checkerboard(9, 9), 8)}
_TRACE, _SIMPLE = {}, {}


def trace(name, corners_only=False):
    if (name, corners_only) not in _TRACE:
        m, connectivity = MAPS[name]
        _TRACE[name, corners_only] = outlines_oracle(m, connectivity, corners_only)
    return _TRACE[name, corners_only]


def simple(name, with_labels, tol, max_rounds=ROUNDS):
    key = (name, with_labels, tol, max_rounds)
    if key not in _SIMPLE:
        o = trace(name)
        _SIMPLE[key] = sr.simplify_oracle(o["vertices"], o["rings"], MAPS[name][0] if with_labels else None, tol, max_rounds)
    return _SIMPLE[key]


def ring_slices(rings):
    return [slice(int(s), int(s) + int(n)) for s, n in zip(rings["start"], rings["count"])]


def dist_exceeds(p, a, b, tolerance):
    """Exact: is p farther than `tolerance` (quantised to 1/16) from the line through a and b (from a when a == b)?"""
    q = Fraction(int(round(tolerance * 16)), 16)
    d, w = b - a, p - a
    len2 = int(d @ d)
    if len2 == 0:
        return Fraction(int(w @ w)) > q * q
    cross = int(d[1]) * int(w[0]) - int(d[0]) * int(w[1])
    return Fraction(cross * cross, len2) > q * q


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("name", list(MAPS))
def test_subsequence_anchors_seeds_and_distance_bound(name, with_labels):
    o = trace(name)
    v = o["vertices"].astype(np.int64)
    anchors = sr.anchor_mask(v, MAPS[name][0] if with_labels else None)
    for tol in TOLERANCES:
        out = simple(name, with_labels, tol)
        assert out["converged"] and out["input_vertex_count"] == len(v) and out["edge_count"] == o["edge_count"]
        k = out["kept"]
        assert (np.diff(k) > 0).all() and (out["vertices"] == o["vertices"][k]).all()       # a subsequence, in input order
        kept = np.zeros(len(v), dtype=bool)
        kept[k] = True
        assert kept[anchors].all()
        for r, sl in enumerate(ring_slices(o["rings"])):
            c, a = v[sl], anchors[sl]
            assert kept[sl][sr.seeds_of(c, a)].all()
            ks = np.flatnonzero(kept[sl])
            assert len(ks) >= 2 and out["rings"]["count"][r] == len(ks) and out["rings"]["start"][r] == kept[:sl.start].sum()
            for i in range(len(ks)):                             # every dropped vertex against the chord it ended in
                lo, hi = ks[i], ks[(i + 1) % len(ks)]
                for p in sr._between(int(lo), int(hi), len(c)):
                    assert not dist_exceeds(c[p], c[lo], c[hi], tol), (name, tol, r, p)
            kc = c[ks]
            area2 = sum(int(kc[i, 1]) * int(kc[(i + 1) % len(kc), 0]) - int(kc[(i + 1) % len(kc), 1]) * int(kc[i, 0]) for i in range(len(kc)))
            assert out["rings"]["area2"][r] == area2 and out["rings"]["collapsed"][r] == (len(kc) < 3 or area2 == 0)
            assert (out["rings"]["y0"][r], out["rings"]["x0"][r]) == tuple(kc.min(0)) and (out["rings"]["y1"][r], out["rings"]["x1"][r]) == tuple(kc.max(0) + 1)
        for f in ("label", "edges", "leader"):
            assert (out["rings"][f] == o["rings"][f]).all()
        assert (out["rings"]["hole"] == (o["rings"]["area2"] < 0)).all()


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("name", list(MAPS))
def test_kept_sets_are_nested_over_tolerances(name, with_labels):
    sets = [set(simple(name, with_labels, tol)["kept"].tolist()) for tol in TOLERANCES]
    for small, large in zip(sets, sets[1:]):
        assert large <= small
    assert len(sets[-1]) < len(sets[0])


@pytest.mark.parametrize("name", list(MAPS))
def test_tolerance_zero_keeps_exactly_the_corners(name):
    """Without labels, on a trace with every lattice vertex: per ring, the kept coordinates are those of the corner trace."""
    full, corners = trace(name), trace(name, corners_only=True)
    out = simple(name, False, 0)
    for a, b in zip(ring_slices(out["rings"]), ring_slices(corners["rings"])):
        assert sorted(map(tuple, out["vertices"][a].tolist())) == sorted(map(tuple, corners["vertices"][b].tolist()))
    assert (out["rings"]["area2"] == full["rings"]["area2"]).all() and not out["rings"]["collapsed"].any()


def _arcs(c, anchors):
    """The arcs of one ring between consecutive anchors, as lists of coordinate tuples (ends included)."""
    ks = np.flatnonzero(anchors)
    return [[tuple(c[p]) for p in [int(ks[i])] + sr._between(int(ks[i]), int(ks[(i + 1) % len(ks)]), len(c)).tolist() + [int(ks[(i + 1) % len(ks)])]]
            for i in range(len(ks))]


@pytest.mark.parametrize("name", ["staircase", "three_labels", "three_labels4", "blobs"])
def test_shared_arcs_agree_from_both_sides(name):
    """Every arc between two anchors that two rings share (the same vertices, in opposite order, in the input) keeps the same
    vertices in both; a ring without two anchors that another ring retraces backwards (an island that fills a hole) keeps
    the same set of coordinates."""
    o = trace(name)
    v = o["vertices"].astype(np.int64)
    lab = MAPS[name][0]
    anchors = sr.anchor_mask(v, lab)
    slices = ring_slices(o["rings"])
    shared = closed = 0
    for tol in TOLERANCES:
        out = simple(name, True, tol)
        kept = np.zeros(len(v), dtype=bool)
        kept[out["kept"]] = True
        arcs = {}                                                # full arc -> the coordinates kept of it, in arc order
        for sl in slices:
            c, k = v[sl], kept[sl]
            if anchors[sl].sum() < 2:
                continue
            ks = np.flatnonzero(anchors[sl])
            for i, arc in enumerate(_arcs(c, anchors[sl])):
                pos = [int(ks[i])] + sr._between(int(ks[i]), int(ks[(i + 1) % len(ks)]), len(c)).tolist() + [int(ks[(i + 1) % len(ks)])]
                arcs.setdefault(tuple(arc), []).append([tuple(c[p]) for p in pos if k[p]])
        for arc, got in arcs.items():
            back = arcs.get(tuple(reversed(arc)))
            if back is not None and arc != tuple(reversed(arc)):
                shared += 1
                assert got[0] == back[0][::-1], (name, tol, arc[:3])
        whole = {}
        for sl in slices:
            if anchors[sl].sum() < 2:
                whole.setdefault(frozenset(map(tuple, v[sl].tolist())), []).append(frozenset(map(tuple, v[sl][kept[sl]].tolist())))
        for sets in whole.values():
            closed += len(sets) > 1
            assert all(s == sets[0] for s in sets)
    assert shared > 0
    if name in ("staircase", "three_labels"):
        assert closed > 0                                        # the island that fills a hole


def test_start_vertex_and_direction_do_not_matter():
    o = trace("blobs")
    v = o["vertices"]
    for r, sl in enumerate(ring_slices(o["rings"])):
        c = v[sl]
        if len(c) < 12:
            continue
        one = {f: a[r:r + 1].copy() for f, a in o["rings"].items()}
        one["start"][:] = 0
        want = None
        for variant in (c, np.roll(c, 5, axis=0), np.roll(c, -3, axis=0)[::-1], c[::-1]):
            for tol in (0.5, 2.5):
                got = sr.simplify_oracle(np.ascontiguousarray(variant), one, None, tol, ROUNDS)
                coords = (tol, frozenset(map(tuple, got["vertices"].tolist())))
                want = want or {}
                assert want.setdefault(tol, coords) == coords


def test_truncation():
    full = simple("spiral", False, 0.5)
    assert full["converged"] and full["rounds"] > 8
    cut = simple("spiral", False, 0.5, 2)
    assert not cut["converged"] and cut["rounds"] == 2
    assert set(cut["kept"].tolist()) < set(full["kept"].tolist())
    exact = simple("spiral", False, 0.5, full["rounds"])
    assert exact["converged"] and exact["rounds"] == full["rounds"] and (exact["kept"] == full["kept"]).all()
    short = simple("spiral", False, 0.5, full["rounds"] - 1)
    assert not short["converged"] and set(short["kept"].tolist()) < set(full["kept"].tolist())


def test_a_vertex_exactly_at_the_tolerance_is_dropped():
    """A triangle whose apex is 3 from its base: dropped at tolerance 3, kept at 3 - 1/16; the tolerance is rounded to 1/16
    with ties to even."""
    v = np.asarray([(0, 0), (0, 10), (3, 5)], dtype=np.int32)   # seed 1 = (0, 0), the smallest; seed 2 = (0, 10), the farthest
    rings = {"ring": np.zeros(1, np.int32), "label": np.ones(1, np.int32), "start": np.zeros(1, np.int32), "count": np.full(1, 3, np.int32),
             "edges": np.full(1, 3, np.int32), "area2": np.full(1, 30, np.int64), "leader": np.zeros(1, np.int32)}
    kept = lambda tol: set(map(tuple, sr.simplify_oracle(v, rings, None, tol, 8)["vertices"].tolist()))
    assert kept(3) == {(0, 0), (0, 10)} and kept(3 - 1 / 16) == {(0, 0), (0, 10), (3, 5)} and kept(0) == kept(3 - 1 / 16)
    assert kept(3 - 1 / 32) == kept(3)                           # 47.5 / 16 rounds to 48 / 16
    assert sr.eps2q_of(1 / 32) == 0 and sr.eps2q_of(3 / 32) == 4 and sm.eps2q(2.5) == sr.eps2q_of(2.5) == 1600
    out = sr.simplify_oracle(v, rings, None, 3, 8)
    assert out["rings"]["collapsed"].all() and out["rings"]["area2"][0] == 0 and out["rounds"] == 0 and out["converged"]


def test_round_trip_of_the_oracle_through_the_reference_rasteriser():
    """What tests/test_simplify_gpu.py relies on: simplified with the label map, the three-label map rasterises without
    overlap at tolerances 0 and 1, and at 0 back to itself."""
    m = MAPS["three_labels"][0]
    for tol in (0, 1):
        table = iu.pack_polygons(iu.to_polygons(simple("three_labels", True, tol)))
        lab, overlap = rr.rasterise(table.edges, *m.shape, dtype=np.int32)
        assert overlap == 0
        assert (lab == m).all() == (tol == 0)


# ---- the Python surface, without a device --------------------------------------------------------------------------------------
def _dict(name="three_labels"):
    o = trace(name)
    return {"vertices": torch.from_numpy(o["vertices"].copy()), "rings": {f: a.copy() for f, a in o["rings"].items()},
            "ring_count": o["ring_count"], "vertex_count": o["vertex_count"], "edge_count": o["edge_count"]}


def test_argument_errors_before_the_device():
    d, lab = _dict(), torch.from_numpy(MAPS["three_labels"][0].copy())
    with pytest.raises(InsarError, match="dict region_outlines returns"):
        iu.simplify_outlines([1, 2], tolerance=1.0)
    with pytest.raises(InsarError, match="must be a torch tensor"):
        iu.simplify_outlines(dict(d, vertices=d["vertices"].numpy()), tolerance=1.0)
    with pytest.raises(InsarError, match="contiguous int32 tensor"):
        iu.simplify_outlines(dict(d, vertices=d["vertices"].long()), tolerance=1.0)
    with pytest.raises(InsarError, match="contiguous int32 tensor"):
        iu.simplify_outlines(dict(d, vertices=d["vertices"].t().contiguous().t()), tolerance=1.0)
    with pytest.raises(InsarError, match="must hold start, count"):
        iu.simplify_outlines(dict(d, rings={"start": d["rings"]["start"]}), tolerance=1.0)
    for tol in (float("nan"), float("inf"), -0.5, 1024.5, "1", True, None):
        with pytest.raises(InsarError, match="tolerance="):
            iu.simplify_outlines(d, tolerance=tol)
    for mr in (0, 4096, 2.0, True):
        with pytest.raises(InsarError, match="max_rounds="):
            iu.simplify_outlines(d, tolerance=1.0, max_rounds=mr)
    with pytest.raises(InsarError, match="labels must be a torch tensor"):
        iu.simplify_outlines(d, MAPS["three_labels"][0], tolerance=1.0)
    with pytest.raises(InsarError, match="contiguous 2-D int32"):
        iu.simplify_outlines(d, lab.long(), tolerance=1.0)
    with pytest.raises(InsarError, match="contiguous 2-D int32"):
        iu.simplify_outlines(d, lab.t(), tolerance=1.0)
    with pytest.raises(InsarError, match="outside the 20 x 48 label map"):
        iu.simplify_outlines(d, lab[:20].contiguous(), tolerance=1.0)
    with pytest.raises(InsarError, match="must tile the vertex array"):
        iu.simplify_outlines(dict(d, vertices=d["vertices"][:-1].contiguous()), tolerance=1.0)
    c = _dict()
    c["rings"]["start"][1] += 1
    with pytest.raises(InsarError, match="must tile the vertex array"):
        iu.simplify_outlines(c, tolerance=1.0)
    # with labels: count == edges, i.e. traced with corners_only=False
    o = trace("three_labels", corners_only=True)
    corners = {"vertices": torch.from_numpy(o["vertices"].copy()), "rings": o["rings"]}
    with pytest.raises(InsarError, match="count == edges"):
        iu.simplify_outlines(corners, lab, tolerance=1.0)
    # everything in order: only the device is missing
    for args in ((d, lab), (d,), (corners,)):
        with pytest.raises(InsarError, match="ROCm tensor"):
            iu.simplify_outlines(*args, tolerance=1.0)


def test_empty_input_gives_an_empty_result():
    o = outlines_oracle(np.zeros((5, 5), dtype=np.int32))
    out = iu.simplify_outlines({"vertices": torch.from_numpy(o["vertices"]), "rings": o["rings"], "edge_count": 0}, tolerance=2.0)
    assert out["vertex_count"] == out["ring_count"] == out["rounds"] == out["input_vertex_count"] == 0 and out["converged"] is True
    assert tuple(out["vertices"].shape) == (0, 2) and tuple(out["kept"].shape) == (0,) and set(out["rings"]) == set(sr.RING_FIELDS)
    assert iu.to_polygons(out) == [] and iu.to_geojson(out)["features"] == []


def test_host_queries_and_abi():
    assert _lib.ABI_VERSION == 8 and _lib.load().insar_version() == 8
    assert [sm.launches(r) for r in (0, 1, 8, 65)] == [10, 14, 42, 270]
    s1, t1 = sm.scratch_bytes(1000, 10)
    s2, t2 = sm.scratch_bytes(2000, 10)
    s3, t3 = sm.scratch_bytes(1000, 20)
    assert t1 == t2 == 48 * 11 and t3 == 48 * 21 and s1 < s2 and s1 < s3 and s1 % 16 == s2 % 16 == 0
    assert 45 * 1000 <= s2 - s1 <= 46 * 1000 + 64               # 45 bytes per vertex and 20 per block of 256
    for mv, mr in ((0, 1), (1, 0), ((1 << 28) + 1, 1), (1, (1 << 26) + 1)):
        with pytest.raises(InsarError, match="outside 1"):
            sm.scratch_bytes(mv, mr)
    assert "SimplifyScratch" in iu.__all__ and "simplify_outlines" in iu.__all__


def test_scratch_bytes_are_what_they_were():
    """The byte counts of the build before the scratch core moved into csrc/dp_common.h: callers size buffers by them."""
    assert sm.scratch_bytes(1, 1) == (16672, 96)
    assert sm.scratch_bytes(1000, 37) == (62592, 1824)
    assert sm.scratch_bytes(70001, 513) == (3186448, 24672)
    assert sm.scratch_bytes(1 << 22, 65536) == (190922768, 3145776)


def test_entry_points_validate_before_the_device():
    """Null pointers, counts against capacities, alignment, the label map's size, eps2q and the round numbers: every one is an
    error code, not a launch. The pointers are never dereferenced on the host."""
    call = _lib.call
    A, B = 1 << 20, 2 << 20                                      # two aligned, never dereferenced addresses
    setup = lambda **k: call("insar_simplify_setup", k.get("v", A), k.get("nv", 100), k.get("r", B), k.get("nr", 3), k.get("lab", None),
                             k.get("H", 0), k.get("W", 0), k.get("vm", 100), k.get("rm", 3), k.get("s", A), None)
    for kw, match in ((dict(v=None), "null pointer \\(vertices\\)"), (dict(r=None), "null pointer \\(rings\\)"), (dict(s=None), "null pointer \\(scratch\\)"),
                      (dict(nv=0), "n_vertices 0"), (dict(nv=101), "n_vertices 101"), (dict(nr=4), "n_rings 4"), (dict(nr=0), "n_rings 0"),
                      (dict(nv=2, nr=3), "3 rings over 2 vertices"), (dict(v=A + 4), "not 8-byte aligned"), (dict(r=B + 8), "not 16-byte aligned"),
                      (dict(vm=0), "max_vertices 0"), (dict(rm=0), "max_rings 0"),
                      (dict(lab=A, H=0, W=5), "label map 0 x 5"), (dict(lab=A, H=5, W=16385), "label map 5 x 16385"), (dict(lab=A + 2, H=5, W=5), "labels not 4-byte")):
        with pytest.raises(InsarError, match=match):
            setup(**kw)
    rounds = lambda **k: call("insar_simplify_rounds", A, 100, B, 3, k.get("q", 256), k.get("first", 0), k.get("n", 8), k.get("mr", 64), 100, 3,
                              k.get("s", A), None)
    for kw, match in ((dict(q=-1), "eps2q -1"), (dict(q=16384 * 16384 + 1), "eps2q"), (dict(mr=0), "max_rounds 0"), (dict(mr=4096), "max_rounds 4096"),
                      (dict(first=-1), "rounds -1"), (dict(n=0), "rounds 0"), (dict(first=60, n=6), "rounds 60"), (dict(s=None), "null pointer")):
        with pytest.raises(InsarError, match=match):
            rounds(**kw)
    finish = lambda **k: call("insar_simplify_finish", A, 100, B, 3, k.get("mr", 64), 100, 3, A, k.get("t", B), k.get("ov", A), k.get("ok", A), None)
    for kw, match in ((dict(t=None), "null pointer \\(table\\)"), (dict(ov=None), "out_vertices"), (dict(ok=None), "out_kept"), (dict(t=B + 8), "table not 16-byte"),
                      (dict(ov=A + 4), "not 8-byte"), (dict(mr=0), "max_rounds 0")):
        with pytest.raises(InsarError, match=match):
            finish(**kw)
    with pytest.raises(InsarError, match="null pointer"):
        call("insar_simplify_scratch_bytes", 10, 10, None, ctypes.byref(ctypes.c_int64()))


# ---- to_polygons(drop_collapsed=...) -------------------------------------------------------------------------------------------
def _hand_made():
    """Label 1: a square with a hole; label 2: an exterior that collapsed to a line with a (collapsed) hole; label 3: a
    collapsed two-vertex ring next to a sound triangle."""
    rings_yx = [[(0, 0), (0, 10), (10, 10), (10, 0)], [(2, 2), (8, 2), (8, 8), (2, 8)],          # label 1
                [(20, 0), (20, 9), (20, 4)], [(20, 2), (20, 3)],                                   # label 2
                [(30, 0), (30, 5)], [(40, 0), (40, 6), (46, 0)]]                                    # label 3
    v = np.asarray([p for r in rings_yx for p in r], dtype=np.int32)
    count = np.asarray([len(r) for r in rings_yx], dtype=np.int32)
    area2 = []
    for r in rings_yx:
        n = len(r)
        area2.append(sum(r[i][1] * r[(i + 1) % n][0] - r[(i + 1) % n][1] * r[i][0] for i in range(n)))
    rings = {"ring": np.arange(6, dtype=np.int32), "label": np.asarray([1, 1, 2, 2, 3, 3], dtype=np.int32),
             "start": (np.cumsum(count) - count).astype(np.int32), "count": count, "area2": np.asarray(area2, dtype=np.int64),
             "hole": np.asarray([False, True, False, True, False, False]), "collapsed": np.asarray([False, False, True, True, True, False])}
    return {"vertices": v, "rings": rings}


def test_to_polygons_drops_collapsed_rings():
    d = _hand_made()
    assert d["rings"]["area2"].tolist()[:2] == [200, -72] and d["rings"]["area2"][2] == 0
    kept = iu.to_polygons(d)
    assert [e["label"] for e in kept] == [1, 3]
    assert len(kept[0]["polygons"]) == 1 and len(kept[0]["polygons"][0]["holes"]) == 1
    assert len(kept[1]["polygons"]) == 1 and kept[1]["polygons"][0]["exterior"][:-1].tolist() == [[40, 0], [40, 6], [46, 0]]
    every = iu.to_polygons(d, drop_collapsed=False)
    assert [e["label"] for e in every] == [1, 2, 3] and len(every[1]["polygons"][0]["holes"]) == 1 and len(every[2]["polygons"]) == 2
    gj = iu.to_geojson(d)
    assert [f["properties"]["label"] for f in gj["features"]] == [1, 3] and all(f["geometry"]["type"] == "Polygon" for f in gj["features"])
    assert len(iu.to_geojson(d, drop_collapsed=False)["features"]) == 3
    # a dict without the field is handled as ever, whatever the keyword says: exteriors and holes by the sign of area2
    plain = {"vertices": d["vertices"], "rings": {f: a for f, a in d["rings"].items() if f != "collapsed"}}
    a, b = iu.to_polygons(plain), iu.to_polygons(plain, drop_collapsed=False)
    assert [e["label"] for e in a] == [e["label"] for e in b] == [1, 3]                  # zero-area rings are neither
    assert len(a[1]["polygons"]) == len(b[1]["polygons"]) == 1 and len(a[0]["polygons"][0]["holes"]) == 1


def test_to_polygons_of_an_oracle_result():
    """Real output: at tolerance 8 half of the three-label map's rings collapse; what is left are sound polygons."""
    out = simple("three_labels", True, 8)
    assert 0 < out["rings"]["collapsed"].sum() < out["ring_count"]
    polys = iu.to_polygons(out)
    n = sum(1 + len(p["holes"]) for e in polys for p in e["polygons"])
    assert n <= out["ring_count"] - out["rings"]["collapsed"].sum()
    assert sum(1 + len(p["holes"]) for e in iu.to_polygons(out, drop_collapsed=False) for p in e["polygons"]) == out["ring_count"]
