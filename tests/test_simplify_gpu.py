"""GPU: outline simplification (insar_unet_ca_amd/simplify.py on csrc/simplify.hip) against the sequential oracle of
tests/simplify_ref.py (pinned by its own invariants in tests/test_simplify_host.py).

Every comparison is bitwise: the kept vertices, their indices, every field of the ring table, the counts, `rounds` and
`converged`. The rings come from `region_outlines` on the device (itself bitwise against its own oracle in
tests/test_outlines_gpu.py). The kernels work in blocks of 256 positions, so the maps (at most 96 x 160, up to 3e4 vertices)
cross more than a hundred of them; the one-work-group carry and prefix scans take 256 blocks = 65 536 positions per pass, and
no map of that size has that many vertices, so two hand-made circle outlines of 7e4 vertices in all cross that boundary as well."""
import numpy as np
import pytest
import torch

from tests import simplify_ref as sr

pytestmark = pytest.mark.gpu
TOLERANCES = (0, 0.5, 1, 2.5, 8)
ROUNDS = 2048                                                    # enough for the spiral to converge
CAPS = dict(max_rings=8192, max_vertices=1 << 16, max_edges=1 << 16)
MAPS = {"checkerboard": (sr.checkerboard(96, 160), 4), "spiral": (sr.spiral(48), 8), "disc": (sr.disc(), 8),
        "ring_island": (sr.ring_with_island(), 8), "staircase": (sr.two_label_staircase(), 8),
        "three_labels": (sr.three_labels(), 8), "blobs": (sr.blobs(), 8), "blobs2": (sr.blobs(seed=6), 4)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_RAW, _ORACLE = {}, {}


def _raw(dev, name):
    """(label tensor, region_outlines with every lattice vertex, the same as numpy) of a map, traced once."""
    if name not in _RAW:
        import insar_unet_ca_amd as iu
        m, connectivity = MAPS[name]
        t = torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)).to(dev)
        raw = iu.region_outlines(t, connectivity=connectivity, corners_only=False, **CAPS)
        _RAW[name] = (t, raw, raw["vertices"].cpu().numpy())
    return _RAW[name]


def _oracle(name, verts, rings, labels, tolerance, max_rounds):
    key = (name, labels is not None, tolerance, max_rounds)
    if key not in _ORACLE:
        _ORACLE[key] = sr.simplify_oracle(verts, rings, labels, tolerance, max_rounds)
    return _ORACLE[key]


def _compare(out, ref, what):
    for k in ("vertex_count", "ring_count", "edge_count", "input_vertex_count", "rounds", "converged"):
        assert out[k] == ref[k] and type(out[k]) is type(ref[k]), f"{what}: {k} {out[k]!r}, oracle {ref[k]!r}"
    assert out["vertices"].dtype == torch.int32 and tuple(out["vertices"].shape) == (ref["vertex_count"], 2), what
    assert out["kept"].dtype == torch.int32 and tuple(out["kept"].shape) == (ref["vertex_count"],), what
    k = out["kept"].cpu().numpy()
    assert k.tobytes() == ref["kept"].tobytes(), f"{what}: kept differs from {np.flatnonzero(k != ref['kept'])[:8]}"
    assert out["vertices"].cpu().numpy().tobytes() == ref["vertices"].tobytes(), f"{what}: vertices differ"
    assert set(out["rings"]) == set(sr.RING_FIELDS), what
    for f in sr.RING_FIELDS:
        got, want = out["rings"][f], ref["rings"][f]
        assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {f} {got.dtype} {got.shape}"
        assert got.tobytes() == want.tobytes(), f"{what}: {f} differs at rings {np.flatnonzero(got != want)[:8]}"


@pytest.mark.parametrize("with_labels", [True, False], ids=["labels", "alone"])
@pytest.mark.parametrize("name", [n for n in MAPS if n != "blobs2"])
def test_maps_against_the_oracle(dev, name, with_labels):
    import insar_unet_ca_amd as iu
    t, raw, verts = _raw(dev, name)
    before_v, before_l = raw["vertices"].clone(), t.clone()
    before_r = {f: a.copy() for f, a in raw["rings"].items()}
    lab = MAPS[name][0] if with_labels else None
    for tol in TOLERANCES:
        ref = _oracle(name, verts, raw["rings"], lab, tol, ROUNDS)
        out = iu.simplify_outlines(raw, t if with_labels else None, tolerance=tol, max_rounds=ROUNDS)
        _compare(out, ref, f"{name} labels {with_labels} tolerance {tol}")
        assert ref["converged"]
        print(f"{name} labels {with_labels} tol {tol}: {ref['input_vertex_count']} -> {ref['vertex_count']} vertices, "
              f"{ref['rounds']} rounds, {int(ref['rings']['collapsed'].sum())} of {ref['ring_count']} rings collapsed")
    assert torch.equal(raw["vertices"], before_v) and torch.equal(t, before_l)            # the inputs are not written
    assert all(raw["rings"][f].tobytes() == before_r[f].tobytes() for f in before_r)


def test_the_maps_are_what_they_claim(dev):
    """Thousands of 4-vertex rings that collapse at tolerance 1; a spiral of one ring over several blocks and hundreds of
    rounds; anchors on the maps with two and three labels; more than one block in every map-sized case."""
    t, raw, verts = _raw(dev, "checkerboard")
    assert raw["ring_count"] == 96 * 160 // 2 and (raw["rings"]["count"] == 4).all() and raw["vertex_count"] > 100 * 256
    ref = _oracle("checkerboard", verts, raw["rings"], None, 1, ROUNDS)
    assert ref["rings"]["collapsed"].all()
    t, raw, verts = _raw(dev, "spiral")
    ref = _oracle("spiral", verts, raw["rings"], None, 0, ROUNDS)
    assert raw["ring_count"] == 1 and raw["vertex_count"] > 8 * 256 and ref["rounds"] > 64
    for name, least in (("staircase", 2), ("three_labels", 6)):
        t, raw, verts = _raw(dev, name)
        assert sr.anchor_mask(verts, MAPS[name][0]).sum() >= least


@pytest.mark.parametrize("max_rounds", [1, 2, 8, 9, 17])
def test_truncation_on_the_spiral(dev, max_rounds):
    """Fewer rounds than the spiral needs: the oracle's result cut at that depth, not converged. 8 is one batch of rounds
    between two looks at the counter, 9 and 17 put the probe into a batch of its own."""
    import insar_unet_ca_amd as iu
    t, raw, verts = _raw(dev, "spiral")
    for with_labels in (True, False):
        ref = _oracle("spiral", verts, raw["rings"], MAPS["spiral"][0] if with_labels else None, 0.5, max_rounds)
        out = iu.simplify_outlines(raw, t if with_labels else None, tolerance=0.5, max_rounds=max_rounds)
        _compare(out, ref, f"spiral max_rounds {max_rounds}")
        assert not out["converged"] and out["rounds"] == max_rounds


def test_reused_scratch_across_maps(dev):
    """One scratch, larger than either input, over two different maps of one size, twice each: identical results."""
    import insar_unet_ca_amd as iu
    sc = iu.SimplifyScratch(1 << 16, 8192, 96, 160, dev)
    assert sc.key() == (1 << 16, 8192, 96, 160)
    for _ in range(2):
        for name, tol in (("blobs", 1), ("checkerboard", 0), ("blobs2", 2.5), ("blobs", 8)):
            t, raw, verts = _raw(dev, name)
            ref = _oracle(name, verts, raw["rings"], MAPS[name][0], tol, ROUNDS)
            out = iu.simplify_outlines(raw, t, tolerance=tol, max_rounds=ROUNDS, scratch=sc)
            _compare(out, ref, f"{name} tolerance {tol} (scratch)")
    from insar_unet_ca_amd._lib import InsarError
    with pytest.raises(InsarError, match="scratch for"):
        iu.simplify_outlines(raw, t, tolerance=1, scratch=iu.SimplifyScratch(100, 8192, 96, 160, dev))


PAD = 4096


def _guarded(nbytes, dev, fill=0xA5):
    g = torch.full((PAD + nbytes + PAD,), fill, dtype=torch.uint8, device=dev)
    return g, g[PAD:PAD + nbytes]


def _intact(g, nbytes, fill=0xA5):
    h = g.cpu().numpy()
    return bool((h[:PAD] == fill).all() and (h[PAD + nbytes:] == fill).all())


def _phases(dev, raw, labels, tolerance, max_rounds, vm, rm):
    """setup, every round in one call and finish with scratch, both tables and both outputs inside guards; the result in the
    shape of simplify_outlines, and whether every guard is intact."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd import simplify as sm
    from insar_unet_ca_amd._lib import call, ptr
    from insar_unet_ca_amd.outlines import RING_DTYPE
    v, rings = raw["vertices"], raw["rings"]
    V, R = int(v.shape[0]), len(rings["start"])
    H, W = labels.shape
    sb, tb = sm.scratch_bytes(vm, rm)
    used = RING_DTYPE.itemsize * (1 + R)
    gs, scratch = _guarded(sb, dev)
    gi, tin = _guarded(used, dev)
    gt, table = _guarded(used, dev)
    gv, out_v = _guarded(8 * V, dev)
    gk, out_k = _guarded(4 * V, dev)
    host = np.zeros(1 + R, dtype=RING_DTYPE)
    for f in ("start", "count", "label", "edges", "leader", "area2"):
        host[f][1:] = rings[f]
    tin.copy_(torch.from_numpy(host.view(np.uint8)))
    s = _lib.stream_ptr()
    call("insar_simplify_setup", ptr(v), V, ptr(tin), R, ptr(labels), H, W, vm, rm, ptr(scratch), s)
    call("insar_simplify_rounds", ptr(v), V, ptr(tin), R, sm.eps2q(tolerance), 0, max_rounds + 1, max_rounds, vm, rm, ptr(scratch), s)
    call("insar_simplify_finish", ptr(v), V, ptr(tin), R, max_rounds, vm, rm, ptr(scratch), ptr(table), ptr(out_v), ptr(out_k), s)
    torch.cuda.synchronize()
    rec = table.cpu().numpy().view(RING_DTYPE)
    head, rec = rec[0], rec[1:]
    kept = int(head["count"])
    assert int(head["label"]) == R and int(head["edges"]) == V
    out = {"ring": np.arange(R, dtype=np.int32)}
    for f in ("label", "start", "count", "edges", "area2", "y0", "x0", "y1", "x1", "leader"):
        out[f] = rec[f].copy()
    out["hole"] = np.asarray(rings["area2"]) < 0
    out["collapsed"] = rec["_pad"] != 0
    res = {"vertices": out_v.view(torch.int32).reshape(-1, 2)[:kept].clone(), "kept": out_k.view(torch.int32)[:kept].clone(),
           "rings": out, "ring_count": R, "vertex_count": kept, "edge_count": int(raw["edge_count"]), "input_vertex_count": V,
           "rounds": int(head["leader"]), "converged": bool(head["start"])}
    # nothing behind the kept vertices is written either
    tail_v, tail_k = out_v[8 * kept:].cpu().numpy(), out_k[4 * kept:].cpu().numpy()
    ok = (_intact(gs, sb) and _intact(gi, used) and _intact(gt, used) and _intact(gv, 8 * V) and _intact(gk, 4 * V)
          and bool((tail_v == 0xA5).all() and (tail_k == 0xA5).all()))
    return res, ok


@pytest.mark.parametrize("tol", [1, 8])
def test_guarded_phase_calls_with_larger_capacities(dev, tol):
    """The three entry points on `blobs` with capacities larger than the input, every buffer between guard patterns: no guard
    and nothing behind the kept vertices is written, and the result is the oracle's. A section of the scratch carved at the
    wrong offset or size shows here first."""
    t, raw, verts = _raw(dev, "blobs")
    V, R = raw["vertex_count"], raw["ring_count"]
    ref = _oracle("blobs", verts, raw["rings"], MAPS["blobs"][0], tol, ROUNDS)
    ph, ok = _phases(dev, raw, t, tol, ROUNDS, vm=V + 77, rm=R + 5)
    assert ok, "a guard was written"
    _compare(ph, ref, f"blobs tolerance {tol} (phases)")


def test_rings_longer_than_one_scan_pass(dev):
    """Two hand-made circle outlines of 37 600 and 32 800 vertices: together more than the 65 536 positions one pass of the
    carry and prefix scans takes, with kept vertices on both sides of that boundary and segments of the second ring across it."""
    import insar_unet_ca_amd as iu
    v, rings = sr.circle_rings([4700, 4100])
    assert len(v) > 65536 + 4096 and rings["start"][1] < 65536 - 4096
    outl = {"vertices": torch.from_numpy(v).to(dev), "rings": rings, "ring_count": 2, "vertex_count": len(v), "edge_count": len(v)}
    for tol in (1, 8):
        ref = _oracle("circles", v, rings, None, tol, ROUNDS)
        out = iu.simplify_outlines(outl, tolerance=tol, max_rounds=ROUNDS)
        _compare(out, ref, f"circles tolerance {tol}")
        print(f"circles tol {tol}: {len(v)} -> {ref['vertex_count']} vertices, {ref['rounds']} rounds")


@pytest.mark.parametrize("tol", [0, 1])
def test_round_trip_through_the_rasteriser(dev, tol):
    """Simplified with the label map, the three-label map goes through to_polygons, pack_polygons and rasterise_polygons
    without one pixel of overlap; at tolerance 0 the raster is the label map. (tests/test_simplify_host.py checks that the
    oracle and the reference rasteriser alone meet both conditions on this map.)"""
    import insar_unet_ca_amd as iu
    t, raw, verts = _raw(dev, "three_labels")
    H, W = t.shape
    out = iu.simplify_outlines(raw, t, tolerance=tol, max_rounds=ROUNDS)
    res = iu.rasterise_polygons(iu.pack_polygons(iu.to_polygons(out)), H, W, dtype=torch.int32, device=dev)
    assert int(res["overlap_pixels"]) == 0
    if tol == 0:
        assert torch.equal(res["labels"], t)
    else:
        assert (res["labels"] != 0).sum() > 0 and not (res["labels"] == 255).any()


def test_detect_with_simplified_outlines(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    scene = np.random.default_rng(4).standard_normal((64, 96)).astype(np.float32)
    pred = iu.ScenePredictor(net, tile=32, overlap=8, batch=4, num_classes=2)
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():                                       # split the class map about evenly (tests/test_outlines_gpu.py)
        net.outc.bias[1] += torch.log(p[0] / p[1]).median()
    kw = dict(connectivity=8, min_area=2)
    plain = pred.detect(scene, outlines=True, **kw)
    det = pred.detect(scene, outlines=True, simplify=1.0, **kw)
    assert "outlines_raw" not in det and set(det) == set(plain)
    for k in ("mask", "conf", "labels", "mask_clean"):
        assert torch.equal(plain[k], det[k]), k
    for k, v in plain["regions"].items():                        # the perimeter among them: it comes from `edges`
        assert v.tobytes() == det["regions"][k].tobytes(), k
    raw = iu.region_outlines(det["labels"], connectivity=8, corners_only=False)
    hand = iu.simplify_outlines(raw, det["labels"], tolerance=1.0)
    o = det["outlines"]
    assert torch.equal(o["vertices"], hand["vertices"]) and torch.equal(o["kept"], hand["kept"])
    assert all(o[k] == hand[k] for k in ("ring_count", "vertex_count", "edge_count", "rounds", "converged", "input_vertex_count"))
    for f, v in hand["rings"].items():
        assert v.tobytes() == o["rings"][f].tobytes(), f
    ref = sr.simplify_oracle(raw["vertices"].cpu().numpy(), raw["rings"], det["labels"].cpu().numpy(), 1.0, 64)
    _compare(o, ref, "detect")
    assert o["vertex_count"] < plain["outlines"]["vertex_count"]
    # detect(outlines=True) alone is what it was: the corner trace of region_outlines
    direct = iu.region_outlines(plain["labels"], connectivity=8)
    assert torch.equal(plain["outlines"]["vertices"], direct["vertices"]) and "collapsed" not in plain["outlines"]["rings"]
    for f, v in direct["rings"].items():
        assert v.tobytes() == plain["outlines"]["rings"][f].tobytes(), f
    one = iu.detect_scene(net, scene, outlines=True, simplify=1.0, tile=32, overlap=8, batch=4, num_classes=2, **kw)
    assert torch.equal(one["outlines"]["vertices"], o["vertices"])
    assert len(iu.to_geojson(o)["features"]) >= 1
    print(f"detect: {det['count']} regions, {plain['outlines']['vertex_count']} corners, {raw['vertex_count']} lattice vertices, "
          f"{o['vertex_count']} after simplify(1.0)")
