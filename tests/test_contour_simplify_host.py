"""No GPU: the sequential oracle of contour simplification (tests/contour_simplify_ref.py) pinned by its own invariants in Python
integers, every refusal of `simplify_contours` and of detect's `simplify` key (none needs a device), and the `collapsed` /
`input_area2` handling of the host helpers on hand-made dicts."""
import numpy as np
import pytest
import torch

from insar_unet_ca_amd import contours as ct
from insar_unet_ca_amd._lib import InsarError
from tests import contour_simplify_ref as cr
from tests.contours_ref import contours_oracle

TOLERANCES = (0, 0.25, 1, 4)
ROUNDS = 4000


RASTERS = {n: c for n, c in cr.raster_cases().items() if n.startswith("48x64")}
MIXED = "48x64 NaN hole, 1 level"
_CACHE = {}


def _contoured(name):
    if name not in _CACHE:
        m, levels = RASTERS[name]
        _CACHE[name] = contours_oracle(m, levels)
    return _CACHE[name]


def _simplified(name, tol):
    if (name, tol) not in _CACHE:
        _CACHE[name, tol] = cr.simplify_contours_oracle(_contoured(name), tol, ROUNDS)
    return _CACHE[name, tol]


def _lines(c):
    v = [(int(y), int(x)) for y, x in c["vertices"]]
    ln = c["lines"]
    return [(v[int(s):int(s) + int(n)], bool(cl)) for s, n, cl in zip(ln["start"], ln["count"], ln["closed"])]


def _kept_local(c, out):
    """Per line of the input c: the kept local positions, from out["kept"] and the line tables."""
    kept = out["kept"].tolist()
    res = []
    for r in range(c["n_lines"]):
        s, n = int(out["lines"]["start"][r]), int(out["lines"]["count"][r])
        res.append([k - int(c["lines"]["start"][r]) for k in kept[s:s + n]])
    return res


@pytest.mark.parametrize("name", list(RASTERS))
def test_dropped_vertices_lie_within_the_tolerance_of_their_chord(name):
    c = _contoured(name)
    assert c["n_lines"] >= 3 and (name != MIXED or ((~c["lines"]["closed"]).any() and c["lines"]["closed"].any()))
    for tol in TOLERANCES:
        out = _simplified(name, tol)
        assert out["converged"] and out["n_lines"] == c["n_lines"] and out["input_n_vertices"] == c["n_vertices"]
        eps2 = cr.eps_of(tol) ** 2
        for (pts, closed), ks in zip(_lines(c), _kept_local(c, out)):
            n = len(pts)
            assert ks == sorted(ks) and (closed or (ks[0] == 0 and ks[-1] == n - 1))          # open-line ends always stay
            pairs = list(zip(ks, ks[1:] + ks[:1])) if closed else list(zip(ks, ks[1:]))
            seen = set(ks)
            for a, b in pairs:
                (ay, ax), (by, bx) = pts[a], pts[b]
                dy, dx = by - ay, bx - ax
                len2 = dy * dy + dx * dx
                for p in cr.interior(a, b, n, closed):
                    py, px = pts[p][0] - ay, pts[p][1] - ax
                    if len2:
                        assert (dx * py - dy * px) ** 2 <= eps2 * len2, (name, tol, a, p, b)
                    else:
                        assert py * py + px * px <= eps2, (name, tol, a, p, b)
                    seen.add(p)
            assert seen == set(range(n))                                                      # every position is kept or dropped


@pytest.mark.parametrize("name", list(RASTERS))
def test_kept_sets_are_nested_over_tolerances(name):
    sets = [set(_simplified(name, tol)["kept"].tolist()) for tol in TOLERANCES]
    for small, large in zip(sets, sets[1:]):
        assert large <= small
    assert len(sets[-1]) < len(sets[0]) <= _contoured(name)["n_vertices"]


def _subdivided(corners, closed, parts=5):
    pts, keep = [], []
    ends = list(zip(corners, corners[1:] + corners[:1])) if closed else list(zip(corners, corners[1:]))
    for (y0, x0), (y1, x1) in ends:
        keep.append(len(pts))
        pts += [(y0 + (y1 - y0) * k // parts, x0 + (x1 - x0) * k // parts) for k in range(parts)]
    if not closed:
        keep.append(len(pts))
        pts.append(corners[-1])
    return pts, keep


def test_at_tolerance_zero_exactly_the_collinear_vertices_go():
    """Corners joined by straight runs of 5 collinear steps: the corners stay, every vertex on a run goes."""
    stairs = [(1000 * k + 500 * (k % 2), 3000 * k) for k in range(9)]
    box = [(500, 500), (500, 40500), (20500, 60500), (30500, 40500), (30500, 500)]
    a, keep_a = _subdivided(stairs, False)
    b, keep_b = _subdivided(box, True)
    c = cr.make_contours([(a, False), (b, True)])
    out = cr.simplify_contours_oracle(c, 0, ROUNDS)
    assert out["kept"].tolist() == keep_a + [len(a) + k for k in keep_b]
    assert out["lines"]["area2"][1] == c["lines"]["area2"][1] and not out["lines"]["collapsed"].any()
    # on rasters whatever goes at tolerance 0 lies exactly on its chord: the chord test above at eps = 0


def test_direction_and_start_do_not_matter():
    """An open line reversed gives the reversed kept set; a ring rotated to another start keeps the same coordinates."""
    c = _contoured(MIXED)
    done = set()
    for (pts, closed), r in zip(_lines(c), range(c["n_lines"])):
        if len(pts) < 8 or closed in done:
            continue
        done.add(closed)
        for tol in (0.25, 1):
            eps2 = cr.eps_of(tol) ** 2
            ks, _, _ = cr.kept_of_line(pts, closed, eps2, ROUNDS)
            if closed:
                for shift in (1, len(pts) // 3, len(pts) - 1):
                    rot = pts[shift:] + pts[:shift]
                    kr, _, _ = cr.kept_of_line(rot, True, eps2, ROUNDS)
                    assert sorted(rot[k] for k in kr) == sorted(pts[k] for k in ks)
            else:
                kr, _, _ = cr.kept_of_line(pts[::-1], False, eps2, ROUNDS)
                assert [len(pts) - 1 - k for k in reversed(kr)] == ks
    assert done == {True, False}


def test_truncation_is_the_full_result_cut_at_that_depth():
    arc = cr.shedding_arc()
    c = cr.make_contours([(arc, False)])
    full = cr.simplify_contours_oracle(c, 0.25, ROUNDS)
    assert full["rounds"] == len(arc) - 2 and full["converged"] and full["n_vertices"] == len(arc)   # one vertex per level
    for mr in (1, 2, 8, 9, 17):
        cut = cr.simplify_contours_oracle(c, 0.25, mr)
        assert not cut["converged"] and cut["rounds"] == mr and cut["n_vertices"] == 2 + mr
        assert set(cut["kept"].tolist()) <= set(full["kept"].tolist())
    assert cr.simplify_contours_oracle(c, 0.25, len(arc) - 2)["converged"]


def test_ties_and_degenerate_chords():
    # two vertices at the same distance on either side of the chord: the smaller (Y, X) wins, whichever comes first
    for order in ([(100, 500), (-100, 1000)], [(-100, 500), (100, 1000)]):
        pts = [(1000, 0)] + [(1000 + dy, x) for dy, x in order] + [(1000, 1500)]
        ks, rounds, _ = cr.kept_of_line(pts, False, 50 ** 2, 1)
        assert [pts[k] for k in ks if 0 < k < 3] == [(900, min(x for dy, x in order if dy < 0))] and rounds == 1
    # duplicate coordinates: the smallest position; a ring whose vertices all coincide has one seed and collapses
    pts = [(0, 0), (300, 100), (300, 100), (0, 200)]
    assert cr.kept_of_line(pts, False, 0, 1)[0] == [0, 1, 3]
    out = cr.simplify_contours_oracle(cr.make_contours([([(5, 5)] * 4, True)]), 0, 8)
    assert out["kept"].tolist() == [0] and out["lines"]["collapsed"].tolist() == [True] and out["rounds"] == 0
    # an open line that returns to its head: the chord is a point and the distance from it decides (500^2 + 300^2 = 340 000)
    loop = [(0, 0), (400, 300), (500, 300), (0, 0)]
    assert cr.kept_of_line(loop, False, 583 ** 2, 8)[0] == [0, 2, 3] and cr.kept_of_line(loop, False, 584 ** 2, 8)[0] == [0, 3]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _host_dict():
    c = cr.make_contours([([(0, 0), (256, 512), (0, 1024)], False), ([(0, 0), (0, 512), (512, 512), (512, 0)], True)])
    c["vertices"] = torch.from_numpy(c["vertices"])
    return c


def _fake_scratch(max_vertices, max_lines, device):
    sc = object.__new__(ct.ContourSimplifyScratch)
    sc.max_vertices, sc.max_lines = max_vertices, max_lines
    sc.scratch = torch.empty(0, dtype=torch.uint8, device=device)
    return sc


def test_refusals_need_no_device():
    good = _host_dict()

    def bad(match, change=None, **kw):
        c = dict(good, lines=dict(good["lines"]))
        if change:
            change(c)
        args = dict(tolerance=1.0)
        args.update(kw)
        with pytest.raises(InsarError, match=match):
            ct.simplify_contours(c, **args)

    with pytest.raises(InsarError, match="must be a dict of the shape contour_lines returns"):
        ct.simplify_contours([1, 2], tolerance=1)
    bad("must be a dict of the shape", lambda c: c.pop("lines"))
    bad("must be a torch tensor", lambda c: c.update(vertices=c["vertices"].numpy()))
    bad(r"contiguous int32 tensor \[V, 2\]", lambda c: c.update(vertices=c["vertices"].to(torch.int64)))
    bad(r"contiguous int32 tensor \[V, 2\]", lambda c: c.update(vertices=c["vertices"].reshape(-1)))
    bad("must hold level, closed, start, count, leader, area2", lambda c: c["lines"].pop("leader"))
    bad("differ in length", lambda c: c["lines"].update(level=c["lines"]["level"][:1]))
    bad("must tile the vertex array", lambda c: c["lines"].update(start=np.array([1, 4], dtype=np.int32)))
    bad("must tile the vertex array", lambda c: c["lines"].update(count=np.array([3, 3], dtype=np.int32)))
    bad("must tile the vertex array", lambda c: c.update(vertices=c["vertices"][:6].contiguous()))
    bad("line 0 is open and has 1 vertices", lambda c: c["lines"].update(start=np.array([0, 1], dtype=np.int32),
                                                                         count=np.array([1, 6], dtype=np.int32)))
    bad("line 1 is closed and has 2 vertices", lambda c: c["lines"].update(start=np.array([0, 5], dtype=np.int32),
                                                                           count=np.array([5, 2], dtype=np.int32)))
    for t in (float("nan"), float("inf"), -0.5, 1024.5):
        bad("tolerance=.*finite, 0 .. 1024", tolerance=t)
    for t in ("1", None, True):
        bad("tolerance=.*a number of pixels", tolerance=t)
    for r in (0, 4096, 2.0, True):
        bad("max_rounds=", max_rounds=r)
    bad("scratch must be a ContourSimplifyScratch", scratch=object())
    bad("scratch for 6 vertices in 2 lines on cpu: the input has 7 vertices in 2 lines on cpu", scratch=_fake_scratch(6, 2, "cpu"))
    bad("scratch for 7 vertices in 1 lines on cpu: the input has 7 vertices in 2 lines", scratch=_fake_scratch(7, 1, "cpu"))
    bad("scratch for 8 vertices in 2 lines on meta: the input has 7 vertices in 2 lines on cpu", scratch=_fake_scratch(8, 2, "meta"))
    bad("must be a ROCm tensor")                                  # a well-formed dict on the host: no CPU fallback
    # an empty input needs no device either, and comes back empty in the same shape
    empty = {"vertices": torch.empty(0, 2, dtype=torch.int32), "lines": {f: np.zeros(0, dtype=np.int32) for f in ct.LINE_FIELDS},
             "levels_q": np.asarray([3], dtype=np.int32), "scale": 1.0, "level_counts": np.zeros(1, dtype=np.int64)}
    out = ct.simplify_contours(empty, tolerance=1)
    assert out["n_lines"] == out["n_vertices"] == out["input_n_vertices"] == out["rounds"] == 0 and out["converged"] is True
    assert set(out["lines"]) == set(ct.SIMPLIFIED_FIELDS) and out["levels_q"] is empty["levels_q"] and tuple(out["kept"].shape) == (0,)
    assert ct.lines_to_coords(out) == [] and ct.contour_polygons(out, 0) == []


def test_detect_refuses_a_bad_simplify_key_before_predict():
    from insar_unet_ca_amd.infer import ScenePredictor
    for t in (-1, 2000.0, float("nan"), "0.5", True):
        with pytest.raises(InsarError, match="contours: simplify="):
            ScenePredictor._contour_kwargs(dict(levels=[0.5], simplify=t))
    kw = ScenePredictor._contour_kwargs(dict(levels=[0.5], smooth=1.5, simplify=0.5))
    assert kw["simplify"] == 0.5 and kw["smooth"] == 1.5
    assert "simplify" not in ScenePredictor._contour_kwargs(dict(levels=[0.5]))


def test_launches_and_scratch_bytes_are_host_arithmetic():
    assert [ct.contour_simplify_launches(r) for r in (-3, 0, 1, 9, 4096, 5000)] == [12, 12, 17, 57, 12 + 5 * 4096, 12 + 5 * 4096]
    sb, tb = ct.contour_simplify_scratch_bytes(1000, 10)
    sb2, tb2 = ct.contour_simplify_scratch_bytes(2000, 10)
    assert tb == tb2 == 48 * 11 and 61 * 1000 < sb - 4 * 4096 < 70 * 1000 + 1024 and sb2 > sb
    for v, l in ((0, 1), (1, 0), ((1 << 28) + 1, 1), (1, (1 << 27) + 1)):
        with pytest.raises(InsarError, match="outside 1.."):
            ct.contour_simplify_scratch_bytes(v, l)
    assert ct.eps_q(0.25) == 64 and ct.eps_q(1024) == 262144 and ct.eps_q(0.001953125) == 0 and ct.eps_q(0.005859375) == 2


def test_scratch_bytes_are_what_they_were():
    """The byte counts of the build before the scratch core moved into csrc/dp_common.h: callers size buffers by them."""
    assert ct.contour_simplify_scratch_bytes(1, 1) == (16704, 96)
    assert ct.contour_simplify_scratch_bytes(1000, 37) == (79040, 1824)
    assert ct.contour_simplify_scratch_bytes(70001, 513) == (4312624, 24672)
    assert ct.contour_simplify_scratch_bytes(1 << 22, 65536) == (258818064, 3145776)


def test_the_long_ring_case_of_the_gpu_suite_is_what_it_claims():
    """The hand-made lines of tests/test_contour_simplify_gpu.py that cross one pass of the one-work-group scans (256 blocks of
    256 positions): sizes, where the ring lies, and how much survives at the two tolerances. The oracle runs here, without a
    device, so that its cost at this size is seen in the host suite."""
    host = cr.scan_pass_lines()
    start, count, V = host["lines"]["start"], host["lines"]["count"], host["n_vertices"]
    assert V > 65536 + 4096 and V <= 70000 and host["lines"]["closed"].tolist() == [False, True, False]
    assert start[1] % 256 != 0 and start[1] < 65536 - 4096 and start[1] + count[1] > 65536 and start[2] % 256 != 0
    for tol in cr.SCAN_PASS_TOLERANCES:
        ref = cr.scan_pass_oracle(tol)
        assert ref["converged"] and ref["input_n_vertices"] == V
        assert min(cr.scan_pass_ring_kept(ref)) >= 2             # the ring keeps vertices on both sides of the boundary
    assert cr.scan_pass_oracle(cr.SCAN_PASS_TOLERANCES[0])["n_vertices"] >= V // 10
    assert cr.scan_pass_oracle(cr.SCAN_PASS_TOLERANCES[1])["n_vertices"] < V // 100


# ---- the host helpers on simplified dicts -------------------------------------------------------------------------------------------
def _square(y, x, side, hole=False):
    pts = [(y, x), (y, x + side), (y + side, x + side), (y + side, x)]
    return pts[::-1] if hole else pts


def _simplified_dict():
    """Hand-made, as `simplify_contours` would return it: a big exterior with a hole, a collapsed exterior (two kept vertices)
    whose hole survived as a sliver, a small exterior that turned over, and an open line."""
    parts = [(_square(0, 0, 25600), True), (_square(2560, 2560, 5120, hole=True), True),
             ([(40000, 0), (40000, 9000)], True), ([(40000, 3000), (40010, 4000), (40000, 5000)], True),
             (_square(30000, 30000, 2560, hole=True), True), ([(100, 30000), (200, 31000), (100, 32000)], False)]
    c = cr.make_contours(parts)
    ln = c["lines"]
    ln["input_area2"] = np.asarray([ln["area2"][0], ln["area2"][1], 999, -5, 77, 0], dtype=np.int64)
    ln["collapsed"] = np.asarray([False, False, True, False, False, False])
    ln["level"][5] = 1
    c["levels_q"] = np.asarray([0, 10], dtype=np.int32)
    assert ln["area2"][4] < 0 and ln["area2"][2] == 0
    c.update(kept=np.arange(c["n_vertices"], dtype=np.int32), input_n_vertices=40, rounds=3, converged=True)
    return c


def test_host_helpers_on_a_simplified_dict():
    c = _simplified_dict()
    coords = ct.lines_to_coords(c)
    assert len(coords) == 5 and [e["closed"] for e in coords] == [True, True, True, True, False]
    assert len(ct.lines_to_coords(c, drop_collapsed=False)) == 6
    assert np.array_equal(ct.lines_to_coords(c, drop_collapsed=False)[2]["xy"], np.array([[0.0, 156.25], [9000 / 256, 156.25]]))
    gj = ct.contours_to_geojson(c)
    assert len(gj["features"]) == 5 and len(ct.contours_to_geojson(c, drop_collapsed=False)["features"]) == 6
    assert gj["features"][0]["geometry"]["coordinates"][0] == gj["features"][0]["geometry"]["coordinates"][-1]
    polys = ct.contour_polygons(c, 0)[0]["polygons"]
    # the exterior with its hole; the ring that turned over is still an exterior by input_area2; the collapsed exterior is gone
    # and took the sliver with it
    assert len(polys) == 2 and [len(p["holes"]) for p in polys] == [1, 0]
    assert np.array_equal(polys[0]["exterior"], np.array(_square(0, 0, 25600) + [(0, 0)]) / 256.0)
    hole = _square(2560, 2560, 5120, hole=True)
    assert np.array_equal(polys[0]["holes"][0], np.array(hole + hole[:1]) / 256.0)
    assert np.array_equal(polys[1]["exterior"][0], np.array([32560, 30000]) / 256.0)
    # without a collapsed exterior a hole that nothing contains is refused as ever
    c["lines"]["collapsed"][2] = False
    c["lines"]["input_area2"][2] = -1
    with pytest.raises(InsarError, match="no ring of positive area of level 0 contains line 2"):
        ct.contour_polygons(c, 0)
    with pytest.raises(InsarError, match="level 1 has 1 open line"):               # open lines are refused as ever
        ct.contour_polygons(c, 1)


def test_a_dict_without_collapsed_takes_the_path_it_took():
    """`contour_lines` dicts: the coordinates, the GeoJSON and the polygons are what the documented rules give, written out
    here, whatever `drop_collapsed` says; area2 decides between exterior and hole."""
    parts = [(_square(0, 0, 2560), True), (_square(512, 512, 1024, hole=True), True), ([(100, 3000), (200, 4000)], False)]
    c = cr.make_contours(parts)
    c["lines"]["level"][2] = 0
    c["levels_q"], c["scale"] = np.asarray([32768], dtype=np.int32), 65536.0
    for kw in ({}, dict(drop_collapsed=True), dict(drop_collapsed=False)):
        coords = ct.lines_to_coords(c, **kw)
        assert [e["level"] for e in coords] == [0, 0, 0] and [e["value"] for e in coords] == [0.5] * 3
        for e, (pts, closed) in zip(coords, parts):
            want = np.ascontiguousarray(np.asarray(pts, dtype=np.float64)[:, ::-1] / 256)
            assert e["closed"] == closed and e["xy"].tobytes() == want.tobytes() and e["xy"].dtype == np.float64
        gj = ct.contours_to_geojson(c, **kw)
        assert [f["geometry"]["coordinates"] for f in gj["features"]] == [
            [[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0], [0.0, 0.0]],
            [[2.0, 6.0], [6.0, 6.0], [6.0, 2.0], [2.0, 2.0], [2.0, 6.0]],
            [[3000 / 256, 100 / 256], [4000 / 256, 200 / 256]]]
    rings_only = cr.make_contours(parts[:2])
    polys = ct.contour_polygons(rings_only, 0)
    assert len(polys) == 1 and polys[0]["label"] == 1 and len(polys[0]["polygons"]) == 1
    p = polys[0]["polygons"][0]
    assert p["exterior"].tobytes() == (np.asarray(parts[0][0] + parts[0][0][:1]) / 256.0).tobytes()
    assert len(p["holes"]) == 1 and p["holes"][0].tobytes() == (np.asarray(parts[1][0] + parts[1][0][:1]) / 256.0).tobytes()
    with pytest.raises(InsarError, match="open line"):
        ct.contour_polygons(c, 0)
