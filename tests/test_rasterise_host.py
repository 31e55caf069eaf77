"""CPU-only: the polygon-rasterisation contract (include/insar_hip.h, "polygon rasterisation"). The scanline restatement of
tests/rasterise_ref.py is pinned by an independent exact rational winding evaluator, by the even-odd rasteriser of
tests/outlines_ref.py on lattice rings, and by the properties the top-left rule promises (watertight fans, translation,
orientation). The packer (insar_unet_ca_amd/rasterise.py) and the host side of the C ABI are checked without a device."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _lib
from insar_unet_ca_amd import rasterise as rs
from insar_unet_ca_amd._lib import InsarError
from tests import rasterise_ref as ref
from tests.outlines_ref import outlines_oracle
from tests.outlines_ref import rasterise as even_odd


def star(rng, cy, cx, rmin, rmax, n):
    """A simple (star-shaped) ring of n vertices on the 1/256 grid round (cy, cx), as float (y, x) that quantise exactly."""
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(rmin, rmax, n)
    return np.stack([np.rint((cy + rad * np.sin(ang)) * 256), np.rint((cx + rad * np.cos(ang)) * 256)], axis=1) / 256.0


def random_scene(rng, H, W, n_poly=3):
    polys = []
    for k in range(n_poly):
        cy, cx = rng.uniform(-2, H + 2), rng.uniform(-2, W + 2)              # some vertices outside the map
        r = rng.uniform(3, 0.6 * max(H, W))
        p = {"exterior": star(rng, cy, cx, 0.5 * r, r, int(rng.integers(3, 9))), "holes": []}
        if k % 2 == 0:
            p["holes"].append(star(rng, cy, cx, 0.1 * r, 0.4 * r, int(rng.integers(3, 7))))
        polys.append({"label": k + 1, "polygons": [p]})
    return polys


@pytest.mark.parametrize("seed", range(6))
def test_scanline_equals_rational_winding(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(5, 25)), int(rng.integers(5, 25))
    table = rs.pack_polygons(random_scene(rng, H, W))
    cover, vsum = ref.cover_vsum(table.edges, H, W)
    for r in range(H):
        for c in range(W):
            assert (int(cover[r, c]), int(vsum[r, c])) == ref.winding_at(table.edges, r, c), (seed, r, c)
    assert cover.max() >= 1 and table.crossings(H) == ref.crossings(table.edges, H)


def speckle(rng, H, W, p=0.55):
    m = (rng.random((H, W)) < p).astype(np.int32) * rng.integers(1, 4, (H, W)).astype(np.int32)
    mid = m[H // 4:3 * H // 4, W // 4:3 * W // 4]                           # a denser block: holes inside regions inside holes
    mid |= 4 * (rng.random(mid.shape) < 0.9).astype(np.int32)
    return m


def nested_rings():
    m = np.zeros((21, 23), dtype=np.int32)
    for k, v in enumerate((5, 0, 5, 0, 7)):                                   # 5 inside its own hole, 7 inside that
        m[1 + 2 * k:20 - 2 * k, 1 + 2 * k:22 - 2 * k] = v
    return m


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["speckle0", "speckle1", "nested"])
def test_lattice_round_trip(name, connectivity):
    labels = nested_rings() if name == "nested" else speckle(np.random.default_rng(int(name[-1])), 26, 31)
    H, W = labels.shape
    oracle = outlines_oracle(labels, connectivity, corners_only=True)
    table = rs.pack_polygons(iu.to_polygons(oracle))
    out, void = ref.rasterise(table.edges, H, W, np.int32)
    assert out.tobytes() == labels.tobytes() and void == 0
    v, rings = oracle["vertices"], oracle["rings"]
    for lab in np.unique(labels[labels != 0]):                                # and ring by ring against the even-odd fill
        mine = [v[s:s + n] for s, n, l in zip(rings["start"], rings["count"], rings["label"]) if l == lab]
        assert (even_odd(mine, H, W) == (out == lab)).all()


@pytest.mark.parametrize("seed", range(12))
def test_fan_is_watertight(seed):
    rng = np.random.default_rng(100 + seed)
    H, W, n = 20, 22, int(rng.integers(3, 10))
    ang = (np.arange(n) + rng.uniform(0.1, 0.9, n)) * 2 * np.pi / n          # convex, and no sliver: the centre is inside
    hull = np.stack([np.rint((10 + 9.5 * np.sin(ang)) * 256), np.rint((11 + 10.5 * np.cos(ang)) * 256)], axis=1) / 256.0
    wts = rng.uniform(0.2, 1.0, n)
    apex = np.rint((wts[:, None] * hull).sum(0) / wts.sum() * 256) / 256.0     # interior: the hull is far wider than 1/256
    fan = [{"label": i + 1, "polygons": [{"exterior": np.stack([apex, hull[i], hull[(i + 1) % n]]), "holes": []}]}
           for i in range(n)]
    whole, _ = ref.cover_vsum(rs.pack_polygons([{"label": 1, "polygons": [{"exterior": hull, "holes": []}]}]).edges, H, W)
    cover, vsum = ref.cover_vsum(rs.pack_polygons(fan).edges, H, W)
    assert set(np.unique(whole)) <= {0, 1} and whole.sum() > 30
    assert (cover == whole).all()                                             # no gap, no double cover
    out, void = ref.decide(cover, vsum)
    assert void == 0 and ((out > 0) == (whole == 1)).all() and out.max() <= n


def _raster(polys, H, W, **kw):
    return ref.rasterise(rs.pack_polygons(polys).edges, H, W, **kw)


def _poly(ring, label=1, holes=()):
    return {"label": label, "polygons": [{"exterior": np.asarray(ring, dtype=np.float64), "holes": [np.asarray(h, dtype=np.float64) for h in holes]}]}


def test_top_left_rule_on_pixel_centres():
    sq = [(1.5, 1.5), (1.5, 4.5), (4.5, 4.5), (4.5, 1.5)]                     # every edge runs through pixel centres
    out, void = _raster([_poly(sq)], 7, 7)
    want = np.zeros((7, 7), dtype=np.uint8)
    want[1:4, 1:4] = 1                                                        # top and left flank in, bottom and right out
    assert out.tobytes() == want.tobytes() and void == 0
    diamond = [(0.5, 2.5), (2.5, 4.5), (4.5, 2.5), (2.5, 0.5)]                # every vertex on a pixel centre
    out, _ = _raster([_poly(diamond)], 6, 6)
    want = np.zeros((6, 6), dtype=np.uint8)
    # the top vertex: both flanks cross row 0 at the same Xi, a span of no width; the bottom vertex's row is not crossed at all
    want[1, 1:3] = 1
    want[2, 0:4] = 1                                                          # the left vertex in, the right vertex out
    want[3, 1:3] = 1
    assert out.tobytes() == want.tobytes()
    two = [_poly([(0, 0), (0, 2.5), (5, 2.5), (5, 0)], 1), _poly([(0, 2.5), (0, 6), (5, 6), (5, 2.5)], 2)]
    out, void = _raster(two, 5, 6)                                            # a shared edge through the centres of column 2
    assert void == 0 and (out[:, :2] == 1).all() and (out[:, 2:] == 2).all()


@pytest.mark.parametrize("seed", range(4))
def test_translation_orientation_and_start_vertex(seed):
    rng = np.random.default_rng(200 + seed)
    H, W = 18, 20
    scene = random_scene(rng, H, W)
    out, void = _raster(scene, H, W)
    dy, dx = int(rng.integers(-5, 6)), int(rng.integers(-5, 6))
    moved = [{"label": e["label"], "polygons": [{"exterior": p["exterior"] + (dy, dx), "holes": [h + (dy, dx) for h in p["holes"]]}
                                                 for p in e["polygons"]]} for e in scene]
    big, _ = _raster(scene, H + 10, W + 10)
    big_moved, _ = _raster([{"label": e["label"], "polygons": [{"exterior": p["exterior"] + (5, 5), "holes": [h + (5, 5) for h in p["holes"]]}
                                                                for p in e["polygons"]]} for e in moved], H + 20, W + 20)
    assert (big_moved[5 + dy:5 + dy + H + 10, 5 + dx:5 + dx + W + 10] == big).all()   # whole-pixel shifts commute
    k = int(rng.integers(1, 3))
    turned = [{"label": e["label"], "polygons": [{"exterior": np.roll(p["exterior"][::-1], k, axis=0),
                                                   "holes": [np.roll(h, k, axis=0) for h in p["holes"]]} for p in e["polygons"]]}
              for e in scene]
    closed = [{"label": e["label"], "polygons": [{"exterior": np.concatenate([p["exterior"], p["exterior"][:1]]), "holes": p["holes"]}
                                                  for p in e["polygons"]]} for e in scene]
    for other in (turned, closed):
        got, gvoid = _raster(other, H, W)
        assert got.tobytes() == out.tobytes() and gvoid == void


def test_overlaps_become_void_and_base_is_kept():
    a, b = _poly([(1, 1), (1, 6), (6, 6), (6, 1)], 3), _poly([(4, 4), (4, 9), (9, 9), (9, 4)], 5)
    out, void = _raster([a, b], 10, 10)
    assert void == 4 and (out[4:6, 4:6] == 255).all() and out[1, 1] == 3 and out[8, 8] == 5 and out[0, 0] == 0
    base = np.arange(100, dtype=np.uint8).reshape(10, 10) % 7 + 10
    out2, void2 = _raster([a, b], 10, 10, base=base, overlap_value=9, fill=77)
    covered = out != 0
    assert void2 == 4 and (out2[~covered] == base[~covered]).all() and (out2[4:6, 4:6] == 9).all() and out2[1, 1] == 3
    # a hole outside its exterior (cover -1), a polygon drawn twice (cover 2) and a self-intersecting bow tie are void too
    lonely = {"label": 2, "polygons": [{"exterior": np.array([(0., 0), (0, 3), (3, 3), (3, 0)]), "holes": [np.array([(5., 5), (5, 8), (8, 8), (8, 5)])]}]}
    out3, void3 = _raster([lonely], 10, 10)
    assert (out3[5:8, 5:8] == 255).all() and void3 == 9
    out4, void4 = _raster([a, a], 10, 10)
    assert void4 == 25 and (out4[1:6, 1:6] == 255).all()
    same, void5 = _raster([_poly([(1, 1), (1, 6), (6, 6), (6, 1)], 3), _poly([(4, 4), (4, 9), (9, 9), (9, 4)], 3)], 10, 10)
    assert void5 == 4                                                         # equal values do not make an overlap unambiguous


def test_dtypes():
    sq = [(0, 0), (0, 4), (4, 4), (4, 0)]
    out, void = _raster([_poly(sq, 70000)], 4, 5, dtype=np.int32)
    assert out.dtype == np.int32 and (out[:, :4] == 70000).all() and void == 0
    out, void = _raster([_poly(sq, 70000)], 4, 5, dtype=np.uint8)
    assert out.dtype == np.uint8 and (out[:, :4] == 255).all() and void == 16     # not representable: void
    out, void = _raster([_poly(sq, 255)], 4, 5)
    assert (out[:, :4] == 255).all() and void == 16                               # the void value itself: void
    out, void = _raster([_poly(sq, -3)], 4, 5, dtype=np.int32, overlap_value=-1)
    assert (out[:, :4] == -3).all() and void == 0
    table = rs.pack_polygons([_poly(sq, 7)], values={7: 300})
    assert (table.edges[:, 4] == 300).all()
    assert (rs.pack_polygons([_poly(sq, 7)], values=lambda l: l + 1).edges[:, 4] == 8).all()
    with pytest.raises(InsarError):
        rs.pack_polygons([_poly(sq, 7)], values={1: 1})
    with pytest.raises(InsarError):
        rs.pack_polygons([_poly(sq, 1 << 31)])


# ---- packing ------------------------------------------------------------------------------------------------------------------
AFFINE = [[3.0, 0.0, 500000.0], [0.0, -3.0, 4100000.0]]                       # integer scale: the float64 round trip is exact


@pytest.mark.parametrize("transform", [None, AFFINE])
def test_geojson_round_trip_gives_the_same_table(transform):
    labels = speckle(np.random.default_rng(5), 20, 24)
    oracle = outlines_oracle(labels, 8, corners_only=True)
    direct = rs.pack_polygons(iu.to_polygons(oracle, transform=transform), transform=transform)
    fc = json.loads(json.dumps(iu.to_geojson(oracle, transform=transform)))
    back = rs.from_geojson(fc, transform=transform)
    assert len(direct) > 100 and back.edges.tobytes() == direct.edges.tobytes()
    assert direct.edges.tobytes() == rs.pack_polygons(iu.to_polygons(oracle)).edges.tobytes()     # the affine cancels exactly
    out, void = ref.rasterise(back.edges, 20, 24, np.int32)
    assert out.tobytes() == labels.tobytes() and void == 0
    assert (back.edges[:, :4] % 256 == 0).all() and direct.bounds[0] >= 0 and direct.bounds[2] <= 20 * 256
    doubled = rs.from_geojson(fc, transform=transform, values=lambda l: 2 * l)
    assert (doubled.edges[:, 4] == 2 * back.edges[:, 4]).all()


def test_packer_drops_degenerate_rings_and_counts_crossings():
    flat = _poly([(1, 1), (1, 5), (1, 9)])                                    # zero area
    back_and_forth = _poly([(1, 1), (4, 4), (1, 1), (4, 4)])
    assert len(rs.pack_polygons([flat, back_and_forth, _poly([(2, 2)]), _poly(np.zeros((0, 2)))])) == 0
    t = rs.pack_polygons([_poly([(0, 0), (0, 4), (3, 4), (3, 0), (0, 0)])])   # closed, with two horizontal edges
    assert len(t) == 2 and (t.edges[:, 1] != t.edges[:, 3]).all() and t.bounds == (0, 0, 768, 1024)
    assert sorted(t.edges[:, 0].tolist()) == [0, 1024] and t.edges.dtype == np.int32
    up = t.edges[t.edges[:, 3] < t.edges[:, 1]]
    assert len(up) == 1 and up[0, 0] == 0                                     # the exterior's left flank runs up: w = +1
    hole = rs.pack_polygons([_poly([(0, 0), (0, 9), (9, 9), (9, 0)], 1, holes=[[(2, 2), (2, 5), (5, 5), (5, 2)]])])
    up = hole.edges[hole.edges[:, 3] < hole.edges[:, 1]]
    assert sorted(up[:, 0].tolist()) == [0, 5 * 256]                          # the hole's RIGHT flank runs up
    rng = np.random.default_rng(9)
    big = rs.pack_polygons(random_scene(rng, 30, 30, 5))
    for H in (1, 7, 30, 100):
        assert big.crossings(H) == ref.crossings(big.edges, H)
    assert t.crossings(2) == 4 and t.crossings(50) == 6 and t.row_value_bound == 2
    v = np.abs(big.edges[:, 4].astype(np.int64))
    lo, hi = np.minimum(big.edges[:, 1], big.edges[:, 3]), np.maximum(big.edges[:, 1], big.edges[:, 3])
    per_row = [int(v[(lo <= 256 * r + 128) & (256 * r + 128 < hi)].sum()) for r in range(-300, 300)]
    assert big.row_value_bound == max(per_row)


def test_packer_rejects_far_coordinates_and_bad_input():
    ok = 65536.0
    assert len(rs.pack_polygons([_poly([(0, 0), (0, ok), (ok, ok)])])) == 2
    with pytest.raises(InsarError, match="65536"):
        rs.pack_polygons([_poly([(0, 0), (0, ok + 1 / 256), (ok, ok)])])
    with pytest.raises(InsarError, match="65536"):
        rs.pack_polygons([_poly([(0, 0), (0, -ok - 1), (ok, ok)])])
    with pytest.raises(InsarError):
        rs.pack_polygons([_poly([(0, 0), (0, float("nan")), (4, 4)])])
    with pytest.raises(InsarError, match="2 x 3"):
        rs.pack_polygons([_poly([(0, 0), (0, 4), (4, 4)])], transform=np.eye(3))
    with pytest.raises(InsarError, match="singular"):
        rs.pack_polygons([_poly([(0, 0), (0, 4), (4, 4)])], transform=[[1, 1, 0], [1, 1, 0]])
    with pytest.raises(InsarError, match="Polygon"):
        rs.from_geojson({"type": "Feature", "properties": {"label": 1}, "geometry": {"type": "Point", "coordinates": [0, 0]}})
    with pytest.raises(InsarError, match="property"):
        rs.from_geojson({"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": []}})
    with pytest.raises(InsarError, match="horizontal"):
        rs.PolygonTable(np.array([[0, 5, 9, 5, 1]]))


# ---- the host side of the C ABI ---------------------------------------------------------------------------------------------
NAMES = ("insar_raster_band_rows", "insar_raster_launches", "insar_raster_scratch_bytes", "insar_raster_polygons")


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 8 and lib.insar_version() == 8
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib._SIGNATURES and name in _lib.EXPORTED_SYMBOLS
    for name in ("PolygonTable", "RasterScratch", "pack_polygons", "from_geojson", "rasterise_polygons", "labels_from_geojson"):
        assert name in iu.__all__ and hasattr(iu, name)


def test_scratch_and_band_queries_without_a_gpu():
    assert rs.launches() == 5
    assert rs.band_rows(1) == 32 and rs.band_rows(4096) == 4 and rs.band_rows(16384) == 1
    prev = 32
    for W in range(1, 16385):
        R = rs.band_rows(W)
        assert R <= prev and R & (R - 1) == 0 and 8 * R * (W + 1) <= 136 * 1024
        prev = R
    a, b = rs.scratch_bytes(64, 96, 1000), rs.scratch_bytes(64, 96, 3000)
    assert a % 16 == 0 and b - a == 8 * 2000 and rs.scratch_bytes(4096, 4096, 1 << 20) >= 8 << 20
    for bad in ((0, 5, 1), (5, 0, 1), (5, 16385, 1), (1 << 17, 16384, 1), (5, 5, -1), (5, 5, (1 << 30) + 1)):
        with pytest.raises(InsarError):
            rs.scratch_bytes(*bad)
    with pytest.raises(InsarError):
        rs.band_rows(16385)
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_raster_scratch_bytes", 5, 5, 1, None)


def test_entry_point_checks_its_arguments_without_a_gpu():
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16                           # 16-byte aligned host memory: never touched
    good = dict(edges=p, n=1, H=8, W=8, cross=4, elem=_lib.RASTER_U8, fill=0, ov=255, base=None, out=p, scratch=p, count=p)

    def go(**kw):
        a = dict(good, **kw)
        _lib.call("insar_raster_polygons", a["edges"], a["n"], a["H"], a["W"], a["cross"], a["elem"], a["fill"], a["ov"], a["base"],
                  a["out"], a["scratch"], a["count"], None)

    for kw, msg in ((dict(H=0), "empty"), (dict(W=16385), "width"), (dict(H=1 << 17, W=16384), "2\\^31"), (dict(cross=-1), "max_crossings"),
                    (dict(n=-1), "n_edges"), (dict(elem=2), "element type"), (dict(fill=256), "0 .. 255"), (dict(ov=-1), "0 .. 255"),
                    (dict(out=None), "null"), (dict(scratch=None), "null"), (dict(count=None), "null"), (dict(edges=None), "null"),
                    (dict(scratch=p + 8), "16-byte"), (dict(count=p + 4), "8-byte"), (dict(edges=p + 2), "4-byte"),
                    (dict(elem=_lib.RASTER_I32, out=p + 2), "4-byte"), (dict(elem=_lib.RASTER_I32, base=p + 1), "4-byte")):
        with pytest.raises(InsarError, match=msg):
            go(**kw)


def test_python_entry_checks_its_arguments_without_a_gpu():
    t = rs.pack_polygons([_poly([(0, 0), (0, 4), (4, 4), (4, 0)])])
    cpu = torch.zeros(8, 8, dtype=torch.uint8)
    for args, kw in (((t, 8, 16385), {}), ((t, 1 << 17, 16384), {}), ((t, 0, 8), {}), ((t, 8, 8), dict(dtype=torch.int64)),
                     ((t, 8, 8), dict(fill=256)), ((t, 8, 8), dict(overlap_value=-1)), ((t, 8, 8), dict(fill=1.5)),
                     ((t.edges, 8, 8), {}), ((t, 8, 8), dict(base=cpu)), ((t, 8, 8), dict(base=cpu.numpy())),
                     ((t, 8, 8), dict(base=torch.zeros(8, 9, dtype=torch.uint8))), ((t, 8, 8), dict(base=cpu.int())),
                     ((t, 8, 8), dict(base=torch.zeros(8, 16, dtype=torch.uint8)[:, ::2])), ((t, 8, 8), dict(device="cpu"))):
        with pytest.raises(InsarError):
            iu.rasterise_polygons(*args, **kw)
    heavy = rs.PolygonTable(np.array([[0, 0, 0, 2560, (1 << 31) - 1], [256, 2560, 256, 0, (1 << 31) - 1], [512, 0, 512, 2560, 5]]))
    with pytest.raises(InsarError, match="2\\^31"):
        iu.rasterise_polygons(heavy, 8, 8, dtype=torch.int32)
