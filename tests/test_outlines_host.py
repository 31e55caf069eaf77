"""CPU-only: the outline oracle's own invariants (tests/outlines_ref.py), the host polygon / GeoJSON helpers on hand-made
ring tables, the InsarRing layout, and the argument checks of region_outlines that need no device."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

from insar_unet_ca_amd import _lib
from insar_unet_ca_amd import outlines as ol
from insar_unet_ca_amd._lib import InsarError
from tests.outlines_ref import outlines_oracle, rasterise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insar_hip.h")


def _label(mask, connectivity):
    structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else None
    return ndimage.label(mask, structure=structure)


def _ring_slices(o):
    r = o["rings"]
    return [o["vertices"][int(s):int(s) + int(c)] for s, c in zip(r["start"], r["count"])]


# ---- the oracle's invariants ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("corners_only", [True, False])
def test_oracle_invariants_on_random_maps(connectivity, corners_only):
    rng = np.random.default_rng(100 + connectivity)
    for trial in range(24):
        H, W = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        mask = rng.random((H, W)) < rng.choice([0.3, 0.5, 0.7])
        labels, n = _label(mask, connectivity)
        labels = labels.astype(np.int32)
        o = outlines_oracle(labels, connectivity, corners_only)
        succ = o["succ"]
        assert sorted(succ.values()) == sorted(succ.keys())                  # a permutation of the boundary edges
        r = o["rings"]
        assert (np.diff(r["leader"]) > 0).all() and o["edge_count"] == int(r["edges"].sum()) == len(succ)
        assert o["vertex_count"] == int(r["count"].sum()) and (r["start"] == np.cumsum(r["count"]) - r["count"]).all()
        if not corners_only:
            assert (r["count"] == r["edges"]).all()
        rings = _ring_slices(o)
        for i in range(1, n + 1):
            mine = np.flatnonzero(r["label"] == i)
            pos = mine[r["area2"][mine] > 0]
            assert len(pos) == 1                                             # one exterior per region ...
            root = int(np.flatnonzero(labels.ravel() == i)[0])
            assert int(r["leader"][pos[0]]) == 4 * root                      # ... led by the top side of its root pixel
            assert int(r["area2"][mine].sum()) == 2 * int((labels == i).sum())
            assert (rasterise([rings[j] for j in mine], H, W) == (labels == i)).all()
        assert (r["hole"] == (r["area2"] < 0)).all() and (r["area2"] != 0).all()


def test_oracle_on_a_hand_checked_map():
    """A 3 x 3 ring of label 5 around a hole: exterior 12 edges / 4 corners / area2 18, hole 4 edges / area2 -2."""
    labels = np.full((3, 3), 5, dtype=np.int32)
    labels[1, 1] = 0
    o = outlines_oracle(labels, 8, True)
    r = o["rings"]
    assert r["label"].tolist() == [5, 5] and r["leader"].tolist() == [0, 4 * 1 + 2]
    assert r["edges"].tolist() == [12, 4] and r["area2"].tolist() == [18, -2] and r["count"].tolist() == [4, 4]
    assert o["vertices"][:4].tolist() == [[0, 0], [0, 3], [3, 3], [3, 0]]
    assert o["vertices"][4:].tolist() == [[1, 2], [1, 1], [2, 1], [2, 2]]      # the hole runs the other way round
    assert (r["y0"].tolist(), r["x0"].tolist(), r["y1"].tolist(), r["x1"].tolist()) == ([0, 1], [0, 1], [4, 3], [4, 3])


def test_saddle_rule():
    labels = np.array([[1, 0], [0, 1]], dtype=np.int32)
    assert outlines_oracle(labels, 8)["ring_count"] == 1 and outlines_oracle(labels, 8)["rings"]["count"][0] == 8
    assert outlines_oracle(labels, 4)["ring_count"] == 2


# ---- to_polygons / to_geojson ----------------------------------------------------------------------------------------------------
def _table(rings):
    """A ring table and vertex array from [(label, [(y, x), ...])], area2 by the shoelace formula."""
    out = {f: [] for f in ("ring", "label", "start", "count", "edges", "area2", "hole", "y0", "x0", "y1", "x1")}
    verts = []
    for i, (label, pts) in enumerate(rings):
        p = np.asarray(pts, dtype=np.int64)
        q = np.roll(p, -1, axis=0)
        a2 = int((p[:, 1] * q[:, 0] - q[:, 1] * p[:, 0]).sum())
        for f, v in (("ring", i), ("label", label), ("start", len(verts)), ("count", len(p)), ("edges", 0), ("area2", a2),
                     ("hole", a2 < 0), ("y0", p[:, 0].min()), ("x0", p[:, 1].min()), ("y1", p[:, 0].max() + 1), ("x1", p[:, 1].max() + 1)):
            out[f].append(v)
        verts.extend(pts)
    rings = {f: np.asarray(v, dtype=np.int64 if f == "area2" else bool if f == "hole" else np.int32) for f, v in out.items()}
    return {"vertices": np.asarray(verts, dtype=np.int32).reshape(-1, 2), "rings": rings, "ring_count": len(rings["ring"]),
            "vertex_count": len(verts), "edge_count": 0}


def _box(y0, x0, y1, x1, hole=False):
    pts = [(y0, x0), (y0, x1), (y1, x1), (y1, x0)]
    return pts if not hole else [pts[1], pts[0], pts[3], pts[2]]


NESTED = [(1, _box(0, 0, 10, 10)),                  # exterior A of label 1
          (1, _box(1, 1, 9, 9, hole=True)),         # its hole
          (1, _box(3, 3, 7, 7)),                    # an island of the same label inside the hole ...
          (1, _box(4, 4, 6, 6, hole=True)),         # ... with a hole of its own
          (2, _box(0, 12, 2, 14)),                  # another label
          (1, _box(0, 20, 5, 25)),                  # a second, separate exterior of label 1 ...
          (1, _box(1, 21, 2, 22, hole=True))]       # ... with a hole


def test_to_polygons_attaches_holes():
    polys = ol.to_polygons(_table(NESTED))
    assert [e["label"] for e in polys] == [1, 2]
    p1 = polys[0]["polygons"]
    assert len(p1) == 3 and [len(p["holes"]) for p in p1] == [1, 1, 1]
    assert p1[0]["holes"][0][0].tolist() == [1, 9] and p1[1]["holes"][0][0].tolist() == [4, 6]
    assert p1[2]["holes"][0][0].tolist() == [1, 22]
    for e in polys:
        for p in e["polygons"]:
            for r in [p["exterior"]] + p["holes"]:
                assert r.shape[1] == 2 and (r[0] == r[-1]).all() and len(r) == 5          # closed
    assert len(polys[1]["polygons"]) == 1 and polys[1]["polygons"][0]["holes"] == []
    assert polys[0]["polygons"][0]["exterior"].dtype == np.int32


def test_to_polygons_single_exterior_and_oracle_round_trip():
    labels = np.zeros((9, 11), dtype=np.int32)
    labels[1:8, 1:10] = 3
    labels[2:4, 2:4] = 0
    labels[4:7, 6:9] = 0
    labels[5, 7] = 3                                 # an island in the second hole: two exteriors under one label
    for conn in (4, 8):
        o = outlines_oracle(labels, conn)
        polys = ol.to_polygons(o)
        assert [e["label"] for e in polys] == [3]
        rings = [r for p in polys[0]["polygons"] for r in [p["exterior"]] + p["holes"]]
        assert (rasterise(rings, 9, 11) == (labels == 3)).all()


def test_transform_and_geojson():
    t = _table(NESTED)
    A = [[30.0, 0.0, 500000.0], [0.0, -30.0, 4100000.0]]               # a north-up raster: x east, y south
    polys = ol.to_polygons(t, transform=A)
    ext = polys[0]["polygons"][0]["exterior"]
    assert ext.dtype == np.float64
    assert ext.tolist() == [[500000.0, 4100000.0], [500300.0, 4100000.0], [500300.0, 4099700.0], [500000.0, 4099700.0],
                            [500000.0, 4100000.0]]
    with pytest.raises(InsarError, match="2 x 3"):
        ol.to_polygons(t, transform=np.eye(3))
    gj = ol.to_geojson(t, properties={1: {"area": 7}, 2: {"name": "b"}})
    back = json.loads(json.dumps(gj))
    assert back == gj and back["type"] == "FeatureCollection" and len(back["features"]) == 2
    f1, f2 = back["features"]
    assert f1["geometry"]["type"] == "MultiPolygon" and f2["geometry"]["type"] == "Polygon"
    assert f1["properties"] == {"label": 1, "area": 7} and f2["properties"] == {"label": 2, "name": "b"}
    assert f2["geometry"]["coordinates"] == [[[12, 0], [14, 0], [14, 2], [12, 2], [12, 0]]]          # [x, y], closed
    assert len(f1["geometry"]["coordinates"]) == 3 and all(len(p) == 2 for p in f1["geometry"]["coordinates"])
    gw = json.loads(json.dumps(ol.to_geojson(t, transform=A, properties=lambda lab: {"twice": 2 * lab})))
    assert gw["features"][1]["geometry"]["coordinates"][0][0] == [500360.0, 4100000.0]
    assert gw["features"][1]["properties"] == {"label": 2, "twice": 4}


# ---- the C ABI without a device ----------------------------------------------------------------------------------------------------
def test_ring_record_layout_matches_the_c_compiler(tmp_path):
    fields = [n for n in ol.RING_DTYPE.names]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(InsarRing));', 'printf("align %zu\\n", _Alignof(InsarRing) );']
    lines += [f'printf("{f} %zu\\n", offsetof(InsarRing, {f}));' for f in fields]
    lines.append("return 0;}")
    src = tmp_path / "ring.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "ring"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == 48 == ol.RING_DTYPE.itemsize
    want = {"area2": 0, "label": 8, "leader": 12, "start": 16, "count": 20, "edges": 24, "y0": 28, "x0": 32, "y1": 36, "x1": 40,
            "_pad": 44}
    for f in fields:
        assert int(got[f]) == want[f] == ol.RING_DTYPE.fields[f][1], f


def test_scratch_query_and_phase_argument_checks():
    sb, tb = ol.scratch_bytes(100, 200, 10, 1000)
    assert tb == 48 * 11 and sb % 16 == 0 and sb >= 100 * 200 * 5 + 1000 * 42
    assert ol.scratch_bytes(100, 200, 10, 2000)[0] > sb
    assert [ol.launches(n) for n in (4, 5, 1024, 1025)] == [16, 18, 32, 34]
    s, t = ctypes.c_int64(0), ctypes.c_int64(0)
    lib = _lib.load()
    bad = [(0, 5, 1, 1), (1 << 15, 1 << 14, 1, 1), (5, 5, 0, 1), (5, 5, 1, 0), (5, 5, 1, (1 << 30) + 1)]
    for H, W, R, E in bad:
        assert lib.insar_outline_scratch_bytes(H, W, R, E, ctypes.byref(s), ctypes.byref(t)) < 0, (H, W, R, E)
    assert lib.insar_outline_scratch_bytes(5, 5, 1, 1, None, ctypes.byref(t)) < 0
    # the phase calls refuse bad arguments before they touch the device (there is none here): null and misaligned buffers,
    # a bad connectivity, an edge count above the capacity
    assert lib.insar_outline_edges(None, 5, 5, 8, 100, 16, 16, None) < 0
    assert lib.insar_outline_edges(16, 5, 5, 6, 100, 16, 16, None) < 0
    assert lib.insar_outline_edges(16, 5, 5, 8, 100, 24, 16, None) < 0
    assert lib.insar_outline_edges(16, 5, 5, 8, 100, 16, None, None) < 0
    assert lib.insar_outline_lead(5, 5, 101, 100, 16, None) < 0
    assert lib.insar_outline_rank(5, 5, -1, 100, 16, None) < 0
    assert lib.insar_outline_rings(16, 5, 5, 10, 0, 100, 16, 16, None) < 0
    assert lib.insar_outline_write(5, 5, 10, 1, 10, 0, 100, 16, 16, 16, None) < 0
    assert lib.insar_outline_write(5, 5, 10, 1, 10, 10, 100, 16, 16, 12, None) < 0
    assert b"insar_outline_write" in lib.insar_last_error()


def test_region_outlines_rejects_bad_arguments_without_a_gpu():
    good = torch.zeros(4, 6, dtype=torch.int32)
    with pytest.raises(InsarError, match="no CPU fallback"):
        ol.region_outlines(good)
    with pytest.raises(InsarError, match="torch tensor"):
        ol.region_outlines(np.zeros((4, 6), dtype=np.int32))
    for bad in (torch.zeros(4, 6, dtype=torch.int64), torch.zeros(4, 6, dtype=torch.uint8), torch.zeros(2, 4, 6, dtype=torch.int32),
                torch.zeros(24, dtype=torch.int32), torch.zeros(6, 4, dtype=torch.int32).t()):
        with pytest.raises(InsarError, match="contiguous 2-D int32"):
            ol.region_outlines(bad)
    with pytest.raises(InsarError, match=r"H \* W < 2\^29"):
        ol.region_outlines(torch.empty(1 << 15, 1 << 14, dtype=torch.int32, device="meta"))
    with pytest.raises(InsarError, match=r"H, W >= 1"):
        ol.region_outlines(torch.zeros(0, 6, dtype=torch.int32))
    for conn in (0, 6, "8", None):
        with pytest.raises(InsarError, match="connectivity"):
            ol.region_outlines(good, connectivity=conn)
    for name in ("max_rings", "max_vertices", "max_edges"):
        for v in (0, -3, 1.5, True, (1 << 30) + 1):
            with pytest.raises(InsarError, match=name):
                ol.region_outlines(good, **{name: v})


def test_exports():
    import insar_unet_ca_amd as iu
    for name in ("region_outlines", "to_polygons", "to_geojson", "OutlineScratch"):
        assert name in iu.__all__ and hasattr(iu, name)
