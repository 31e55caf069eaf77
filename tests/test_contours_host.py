"""CPU-only: the sequential oracle of contour lines (tests/contours_ref.py) pinned by its own invariants (the segment table of
DESIGN.md, exact fractions, point-in-polygon topology, contourpy), and everything of insar_unet_ca_amd/contours.py that needs
no device: the refusals, the byte and launch queries, coordinates, polygons and GeoJSON."""
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from insar_unet_ca_amd import contours as ct
from insar_unet_ca_amd._lib import InsarError
from tests.contours_ref import (bordered, cell_segments, contours_oracle, crossing_offset, inside_even_odd, quantise, smooth_map)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rings(c, level):
    ln = c["lines"]
    return [[tuple(int(t) for t in v) for v in c["vertices"][ln["start"][i]:ln["start"][i] + ln["count"][i]]]
            for i in range(c["n_lines"]) if ln["level"][i] == level]


# ---- the 16 cell masks ------------------------------------------------------------------------------------------------------------
def _design_table():
    """mask (and "joined" / "cut") -> set of segments, parsed from the table of DESIGN.md's "Contour lines" section."""
    txt = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec = txt[txt.index("## Contour lines"):]
    rows = re.findall(r"^\| *(\d+)( joined| cut)? *\|[^|\n]*\| *([^|\n]*?) *\|$", sec, flags=re.M)
    return {(int(m), how.strip()): set(s.replace("→", "").replace(" ", "") for s in seg.split(",") if s.strip() not in ("", "none"))
            for m, how, seg in rows}


def _two_by_two(mask, cut=False):
    """int32 2 x 2 map whose nodes TL, TR, BR, BL are above level 5 as the bits 1, 2, 4, 8 of `mask` say; a saddle is joined
    with below nodes at 0 (sum 20 >= 20) and cut apart with below nodes at -2 (sum 16 < 20)."""
    hi, lo = 10, (-2 if cut else 0)
    v = [hi if mask >> b & 1 else lo for b in range(4)]
    return np.array([[v[0], v[1]], [v[3], v[2]]], dtype=np.int32)


def test_the_sixteen_cell_masks_match_the_table_of_design_md():
    table = _design_table()
    assert len(table) == 18, sorted(table)
    name = {0: "T", 4: "B", 1: "L", 3: "R"}                         # crossing ids of a 2 x 2 map at level 0: T 0, L 1, R 3, B 4
    for mask in range(16):
        for cut in ((False, True) if mask in (5, 10) else (False,)):
            c = contours_oracle(_two_by_two(mask, cut), [5])
            got = {name[a] + name[b] for a, b in c["succ"].items()}
            assert got == table[(mask, ("cut" if cut else "joined") if mask in (5, 10) else "")], (mask, cut, got)
            assert c["n_vertices"] == 2 * len(got) and c["n_lines"] == len(got) and not c["lines"]["closed"].any()
            m = _two_by_two(mask, cut)
            assert set(cell_segments(int(m[0, 0]), int(m[0, 1]), int(m[1, 1]), int(m[1, 0]), 5)) == got
    # the above side lies on the right: T -> L keeps TL, at its right-hand side
    c = contours_oracle(_two_by_two(1), [5])
    (y0, x0), (y1, x1) = c["vertices"]
    assert (y0, x0) == (128, 128 + 128) and (y1, x1) == (128 + 128, 128)
    cross = (x1 - x0) * (128 - y0) - (y1 - y0) * (128 - x0)          # z of d x (TL - start), x right and y down
    assert cross > 0                                                 # positive: TL lies clockwise of d on the screen, its right


def test_maps_without_a_cell_hold_no_lines():
    rng = np.random.default_rng(0)
    for shape in ((1, 64), (64, 1), (1, 1)):
        c = contours_oracle(rng.integers(0, 10, size=shape).astype(np.int32), [3, 6])
        assert c["n_lines"] == 0 and c["n_vertices"] == 0 and c["level_counts"].tolist() == [0, 0]
    c = contours_oracle(np.full((7, 9), 5, dtype=np.int32), [5])     # everywhere equal to the level: all above
    assert c["n_lines"] == 0 and c["n_vertices"] == 0


def test_peak_and_pit():
    peak = np.zeros((3, 3), dtype=np.int32)
    peak[1, 1] = 10
    for m, sign in ((peak, 1), (10 - peak, -1)):
        c = contours_oracle(m, [5])
        assert c["n_lines"] == 1 and c["lines"]["closed"][0] and c["lines"]["count"][0] == 4
        assert np.sign(c["lines"]["area2"][0]) == sign and abs(c["lines"]["area2"][0]) == 2 * 2 * 128 * 128 * 1
        assert c["lines"]["leader"][0] == min(c["succ"])
        assert (c["lines"]["y0"][0], c["lines"]["x0"][0], c["lines"]["y1"][0], c["lines"]["x1"][0]) == (256, 256, 513, 513)


# ---- crossing positions ------------------------------------------------------------------------------------------------------------
def test_positions_against_exact_fractions():
    rng = np.random.default_rng(1)
    for trial in range(2000):
        big = trial % 3 == 0
        lo, hi = (-(1 << 31) + 1, (1 << 31) - 1) if big else (-300, 300)
        qb, qa = sorted(int(v) for v in rng.integers(lo, hi, size=2, endpoint=True))
        if qa == qb:
            continue
        q_l = int(rng.integers(qb + 1, qa, endpoint=True))           # below < level <= above
        f = Fraction(q_l - qb, qa - qb) * 256
        s = (f.numerator * 2 + f.denominator) // (2 * f.denominator)    # round half up: floor(f + 1/2)
        s = min(max(s, 1), 255)
        assert crossing_offset(qb, qa, q_l) == s                     # p is the below end
        assert crossing_offset(qa, qb, q_l) == 256 - s               # p is the above end
    assert crossing_offset(0, 7, 7) == 255                           # q == q_l counts as above: the clamp keeps the vertex off the node
    assert crossing_offset(7, 0, 7) == 1 and crossing_offset(0, 1 << 20, 1) == 1 and crossing_offset(0, 2, 1) == 128


def test_positions_on_a_random_integer_map():
    rng = np.random.default_rng(2)
    m = rng.integers(-50, 50, size=(9, 11)).astype(np.int32)
    c = contours_oracle(m, [-7, 0, 13])
    H, W = m.shape
    ids = sorted(set(c["succ"]) | set(c["pred"]))
    assert len(ids) == c["n_vertices"] and c["level_counts"].sum() == len(ids)
    pos = {}
    for i in range(c["n_lines"]):
        s, n, lead = (int(c["lines"][f][i]) for f in ("start", "count", "leader"))
        k = lead
        for j in range(n):
            pos[k] = tuple(int(t) for t in c["vertices"][s + j])
            k = c["succ"].get(k)
    assert sorted(pos) == ids                                        # every crossing exactly once
    for i, (Y, X) in pos.items():
        l, p, o = i // (2 * H * W), (i // 2) % (H * W), i & 1
        y, x = divmod(p, W)
        a, b = int(m[y, x]), int(m[y + 1, x] if o else m[y, x + 1])
        q_l = int(c["levels_q"][l])
        assert (a >= q_l) != (b >= q_l)
        f = Fraction(q_l - min(a, b), abs(a - b)) * 256
        s = min(max((f.numerator * 2 + f.denominator) // (2 * f.denominator), 1), 255)
        off = s if a < b else 256 - s
        assert (Y, X) == (256 * y + 128 + (off if o else 0), 256 * x + 128 + (0 if o else off))
    assert len(set(pos.values())) == len(pos)                        # distinct crossings, distinct points (levels included)


# ---- topology ------------------------------------------------------------------------------------------------------------------------
def _speckle(H, W, seed):
    return np.random.default_rng(seed).integers(0, 100, size=(H, W)).astype(np.int32)


@pytest.mark.parametrize("case", ["smooth 21x26", "smooth 17x30", "speckle 14x17", "speckle 12x19"])
def test_rings_separate_above_from_below(case):
    kind, shape = case.split()
    H, W = (int(t) for t in shape.split("x"))
    if kind == "smooth":
        m, levels, kw = bordered(smooth_map(H, W, H, amp=50.0), -1000.0), [-20.0, 0.003, 11.5], dict(scale=64.0)
    else:
        m, levels, kw = bordered(_speckle(H, W, W), -1), [20, 50, 51, 90], {}
    c = contours_oracle(m, levels, **kw)
    q, ok = quantise(m, kw.get("scale", 1.0))
    assert ok.all() and c["lines"]["closed"].all() and c["n_lines"] >= len(levels)
    assert (np.diff(c["lines"]["leader"]) > 0).all() and (np.diff(c["lines"]["level"]) >= 0).all()
    for l, q_l in enumerate(c["levels_q"]):
        rings = _rings(c, l)
        for y in range(H):
            for x in range(W):
                assert inside_even_odd(rings, 256 * y + 128, 256 * x + 128) == (q[y, x] >= q_l), (case, l, y, x)
    # the signed areas of a level add up to twice the area of its polygons, which holds every above node's centre
    assert all((c["lines"]["area2"][c["lines"]["level"] == l].sum() > 0) == bool((q >= q_l).any()) for l, q_l in enumerate(c["levels_q"]))


# ---- contourpy ---------------------------------------------------------------------------------------------------------------------
def _integer_map(kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "cone":
        y, x = np.mgrid[:23, :29]
        m = np.clip(np.rint(240 - 14 * np.hypot(y - 9.3, x - 17.7)), 0, 255)
    elif kind == "ramp":
        y, x = np.mgrid[:19, :31]
        m = np.clip(3 * x + 5 * y, 0, 255)
    else:
        m = rng.integers(0, 256, size=(16, 21))
    return m.astype(np.float32)


def _saddle_free(m, levels):
    a = [m >= v for v in levels]
    return not any(((g[:-1, :-1] == g[1:, 1:]) & (g[:-1, 1:] == g[1:, :-1]) & (g[:-1, :-1] != g[:-1, 1:])).any() for g in a)


@pytest.mark.parametrize("kind", ["cone", "ramp", "noise"])
def test_crossing_points_match_contourpy(kind):
    contourpy = pytest.importorskip("contourpy")
    m = _integer_map(kind, 5)
    levels = [20.5, 100.5, 127.5, 200.5]
    c = contours_oracle(m, levels, scale=2.0)
    assert c["levels_q"].tolist() == [41, 201, 255, 401] and (quantise(m, 2.0)[0] == 2 * m).all()
    gen = contourpy.contour_generator(z=m.astype(np.float64))
    tol = 1.0 / 512 + 1e-9
    v = c["vertices"].astype(np.float64)
    for l, level in enumerate(levels):
        theirs = gen.lines(level)
        closed = [len(t) > 2 and (t[0] == t[-1]).all() for t in theirs]
        pts = np.concatenate([t[:-1] if cl else t for t, cl in zip(theirs, closed)] or [np.zeros((0, 2))])      # (x, y) at nodes
        sel = np.concatenate([np.arange(s, s + n) for s, n, lv in zip(c["lines"]["start"], c["lines"]["count"], c["lines"]["level"])
                              if lv == l] or [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        mine = (v[sel][:, ::-1] - 128.0) / 256.0
        assert len(mine) == len(pts) == c["level_counts"][l], (kind, level, len(mine), len(pts))
        if len(mine):
            d = np.abs(mine[:, None, :] - pts[None, :, :]).max(axis=2)
            assert d.min(axis=1).max() <= tol and d.min(axis=0).max() <= tol, (kind, level, d.min(axis=1).max())
        if kind != "noise":
            assert _saddle_free(m, [level])
            mine_closed = c["lines"]["closed"][c["lines"]["level"] == l]
            assert (int(mine_closed.sum()), int((~mine_closed).sum())) == (sum(closed), len(closed) - sum(closed)), (kind, level)
    assert kind == "noise" or _saddle_free(m, levels)
    assert kind != "noise" or not _saddle_free(m, levels)


# ---- open lines ----------------------------------------------------------------------------------------------------------------------
def test_open_lines_on_a_map_with_no_data():
    m = smooth_map(24, 31, 9, amp=60.0)
    m[5:9, 11:16] = np.nan
    m[0, 0] = np.nan
    c = contours_oracle(m, [-15.0, 0.0, 12.0], scale=256.0)
    ln = c["lines"]
    assert (~ln["closed"]).sum() >= 3 and c["n_lines"] > 4
    assert (np.diff(ln["leader"]) > 0).all()
    seen = []
    for i in range(c["n_lines"]):
        k, walk = int(ln["leader"][i]), []
        for _ in range(int(ln["count"][i])):
            walk.append(k)
            k = c["succ"].get(k)
        if ln["closed"][i]:
            assert k == ln["leader"][i] and min(walk) == ln["leader"][i] and ln["area2"][i] != 0
        else:
            assert k is None and walk[0] not in c["pred"] and walk[-1] not in c["succ"] and ln["area2"][i] == 0
            assert ln["count"][i] >= 2
        seen += walk
    assert sorted(seen) == sorted(set(c["succ"]) | set(c["pred"])) and len(seen) == c["n_vertices"]
    # the valid plane and nodata act as NaN does
    holes = np.isnan(m)
    filled = np.where(holes, np.float32(-9999.0), m)
    for kw in (dict(valid=(~holes).astype(np.uint8)), dict(nodata=-9999.0)):
        d = contours_oracle(filled, [-15.0, 0.0, 12.0], scale=256.0, **kw)
        assert d["vertices"].tobytes() == c["vertices"].tobytes() and all(d["lines"][f].tobytes() == ln[f].tobytes() for f in ln)


# ---- refusals and queries: no device -------------------------------------------------------------------------------------------
def test_argument_refusals():
    r = torch.zeros(8, 9)
    ok = dict(levels=[0.5])
    bad = [
        (dict(raster=r.double(), **ok), "raster must be float32 or uint8 or int32"),
        (dict(raster=r[None], **ok), "raster must be 2-D"),
        (dict(raster=r.t(), **ok), "raster must be contiguous"),
        (dict(raster=np.zeros((3, 3)), **ok), "raster must be a torch tensor"),
        (dict(raster=r, levels=[0.5, 0.25]), "strictly increasing after quantisation"),
        (dict(raster=r, levels=[0.5, 0.5 + 1e-9]), r"levels\[1\]=.* -> 32768"),
        (dict(raster=r.to(torch.uint8), levels=[3.2, 3.4]), "strictly increasing"),
        (dict(raster=r, levels=list(range(33))), "1..32 finite numbers"),
        (dict(raster=r, levels=[]), "1..32 finite numbers"),
        (dict(raster=r, levels=[float("nan")]), "1..32 finite numbers"),
        (dict(raster=r, levels="half"), "1..32 finite numbers"),
        (dict(raster=r, scale=0.0, **ok), "scale=0.0: a positive finite number"),
        (dict(raster=r, valid=torch.ones(8, 9), **ok), "valid must be a contiguous 2-D uint8"),
        (dict(raster=r, valid=torch.ones(9, 8, dtype=torch.uint8), **ok), r"valid \(9, 8\): expected \(8, 9\)"),
        (dict(raster=r, nodata=float("nan"), **ok), "nodata is NaN"),
        (dict(raster=r.to(torch.uint8), nodata=300, **ok), "nodata=300 is no value"),
        (dict(raster=r, max_vertices=0, **ok), "max_vertices=0"),
        (dict(raster=r, max_lines=2.0, **ok), "max_lines=2.0"),
        (dict(raster=r, **ok), r"raster must be a ROCm tensor \(no CPU fallback\)"),     # every other check passed
    ]
    for kw, msg in bad:
        kw = dict(kw)
        raster, levels = kw.pop("raster"), kw.pop("levels")
        with pytest.raises(InsarError, match="contour_lines: .*" + msg):
            ct.contour_lines(raster, levels, **kw)
    with pytest.raises(InsarError, match=r"levels \* H \* W = 2 \* 256 \* 2097152 must stay below 2\^30"):
        ct._check_args(torch.empty((256, 1 << 21), dtype=torch.uint8, device="meta"), [1, 2], 1.0, None, None, 1, 1)
    with pytest.raises(InsarError, match=r"need 1 <= H, W <= 2\^22"):
        ct._check_args(torch.empty((1, (1 << 22) + 1), dtype=torch.uint8, device="meta"), [1], 1.0, None, None, 1, 1)


def test_byte_and_launch_queries():
    assert [ct.launches(n) for n in (0, 1, 2, 3, 1024, 1025)] == [5, 11, 13, 15, 31, 33]
    H, W, L, lines, verts = 33, 67, 3, 100, 1000
    sb, tb = ct.scratch_bytes(H, W, L, lines, verts)
    up = lambda b: (b + 15) & ~15
    N, nq = H * W, (H * W + 3) // 4
    nblk, eblk = (nq + 255) // 256, (verts + 1023) // 1024
    want = (up(4 * N) + up(N) + 2 * up(4 * L * nq) + up(4 * L * nblk) + 2 * up(4 * verts) + up(8 * verts) + up(verts) + 2 * up(4 * verts)
            + 2 * up(8 * verts) + up(4 * verts) + 2 * up(4 * eblk))
    assert (sb, tb) == (want, 48 * (4 + lines))
    per_crossing = (ct.scratch_bytes(H, W, L, lines, verts + 1024)[0] - sb) / 1024
    assert per_crossing == 45
    for args, msg in (((0, 5, 1, 1, 1), "H, W in 1"), ((5, 5, 0, 1, 1), "n_levels 0"), ((5, 5, 33, 1, 1), "n_levels 33"),
                      ((1 << 15, 1 << 15, 1, 1, 1), "2\\^30 or more"), ((5, 5, 1, 0, 1), "max_lines 0"), ((5, 5, 1, 1, 0), "max_vertices 0")):
        with pytest.raises(InsarError, match="insar_contour_scratch_bytes: .*" + msg):
            ct.scratch_bytes(*args)


# ---- host helpers ------------------------------------------------------------------------------------------------------------------
def _island_in_a_hole():
    m = np.zeros((13, 15), dtype=np.int32)
    m[1:12, 1:14] = 9
    m[3:10, 3:12] = 0
    m[5:8, 5:10] = 9
    m[6, 7] = 0
    return m


def test_contour_polygons_attach_holes_and_refuse_open_lines():
    m = _island_in_a_hole()
    c = contours_oracle(m, [5])
    assert c["n_lines"] == 4 and sorted(np.sign(c["lines"]["area2"]).tolist()) == [-1, -1, 1, 1]
    (entry,) = ct.contour_polygons(c, 0)
    assert entry["label"] == 1 and len(entry["polygons"]) == 2
    outer, island = sorted(entry["polygons"], key=lambda p: -len(p["exterior"]))
    assert len(outer["holes"]) == 1 and len(island["holes"]) == 1
    assert (outer["exterior"][0] == outer["exterior"][-1]).all() and outer["exterior"].dtype == np.float64
    assert len(island["holes"][0]) == 5 and len(outer["holes"][0]) > len(island["exterior"])     # the pit of one node; the big hole
    assert (np.asarray(outer["exterior"]) * 256 == np.rint(np.asarray(outer["exterior"]) * 256)).all()
    # even-odd over the polygons' rings gives the map back
    rings = [[(int(y * 256), int(x * 256)) for y, x in r[:-1]] for p in entry["polygons"] for r in [p["exterior"]] + p["holes"]]
    for y in range(m.shape[0]):
        for x in range(m.shape[1]):
            assert inside_even_odd(rings, 256 * y + 128, 256 * x + 128) == (m[y, x] >= 5)
    opened = contours_oracle(m[:, 2:], [5])                          # the outer band now runs into the border
    assert not opened["lines"]["closed"].all()
    with pytest.raises(InsarError, match=r"contour_polygons: level 0 has \d+ open line"):
        ct.contour_polygons(opened, 0)
    with pytest.raises(InsarError, match="level_index=1"):
        ct.contour_polygons(c, 1)
    assert ct.contour_polygons(contours_oracle(np.zeros((4, 4), dtype=np.int32), [5]), 0) == []


def test_coordinates_and_geojson():
    m = _island_in_a_hole().astype(np.float32) / 9
    m[0, 3] = 1.0                                                    # a corner cut at the border: an open line
    c = contours_oracle(m, [0.25, 0.5], scale=1024.0)
    lines = ct.lines_to_coords(c)
    assert len(lines) == c["n_lines"] and [e["level"] for e in lines] == c["lines"]["level"].tolist()
    assert {e["value"] for e in lines} == {0.25, 0.5} and any(not e["closed"] for e in lines)
    first = lines[0]["xy"]
    assert first.dtype == np.float64 and (first == c["vertices"][:len(first), ::-1] / 256.0).all()
    A = np.array([[30.0, 0.0, 5e5], [0.0, -30.0, 4e6]])
    world = ct.lines_to_coords(c, A)
    assert np.allclose(world[0]["xy"], np.stack([5e5 + 30 * first[:, 0], 4e6 - 30 * first[:, 1]], axis=1), rtol=0, atol=1e-6)
    with pytest.raises(InsarError, match="2 x 3 affine"):
        ct.lines_to_coords(c, np.eye(3))
    fc = ct.contours_to_geojson(c, A)
    back = json.loads(json.dumps(fc))
    assert back == fc and back["type"] == "FeatureCollection" and len(back["features"]) == c["n_lines"]
    for f, e in zip(back["features"], world):
        xy = np.asarray(f["geometry"]["coordinates"])
        assert f["geometry"]["type"] == "LineString" and f["properties"] == {"level": e["level"], "value": e["value"], "closed": e["closed"]}
        assert len(xy) == len(e["xy"]) + e["closed"] and (xy[:len(e["xy"])] == e["xy"]).all()
        assert not e["closed"] or (xy[0] == xy[-1]).all()
