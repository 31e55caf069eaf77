"""GPU: region outlines (insar_unet_ca_amd/outlines.py on csrc/outline.hip) against the sequential oracle of
tests/outlines_ref.py (pinned by its own invariants in tests/test_outlines_host.py).

Every comparison is bitwise: the ring table, the vertex array and the three counts, with corners_only on and off and
connectivity 4 and 8 on every map. The maps are small: a numbering block is 1024 pixels / edges and a reduction block 256
positions, so 96 x 160 (15 pixel blocks, ~1.5e4 edges) crosses every block boundary there is."""
import numpy as np
import pytest
import torch

from tests.outlines_ref import RING_FIELDS, outlines_oracle, perimeter_by_label, rasterise

pytestmark = pytest.mark.gpu
FIELDS = RING_FIELDS + ("leader",)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _compare(out, ref, what):
    for k in ("edge_count", "ring_count", "vertex_count"):
        assert out[k] == ref[k], f"{what}: {k} {out[k]}, oracle {ref[k]}"
    assert out["vertices"].dtype == torch.int32 and tuple(out["vertices"].shape) == (ref["vertex_count"], 2)
    for f in FIELDS:
        got, want = out["rings"][f], ref["rings"][f]
        assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {f} {got.dtype} {got.shape}"
        assert got.tobytes() == want.tobytes(), f"{what}: {f} differs at rings {np.flatnonzero(got != want)[:8]}"
    v = out["vertices"].cpu().numpy()
    assert v.tobytes() == ref["vertices"].tobytes(), f"{what}: vertices differ from row {np.flatnonzero((v != ref['vertices']).any(1))[:8]}"


_ORACLE = {}


def _oracle(name, labels, connectivity, corners_only):
    key = (name, connectivity, corners_only)
    if key not in _ORACLE:
        _ORACLE[key] = outlines_oracle(labels, connectivity, corners_only)
    return _ORACLE[key]


def _check_all(dev, name, labels):
    """Both connectivities, corners on and off, bitwise against the oracle."""
    import insar_unet_ca_amd as iu
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    t = torch.from_numpy(labels).to(dev)
    for connectivity in (4, 8):
        for corners_only in (True, False):
            ref = _oracle(name, labels, connectivity, corners_only)
            out = iu.region_outlines(t, connectivity=connectivity, corners_only=corners_only, max_rings=4096,
                                     max_vertices=1 << 16, max_edges=1 << 16)
            _compare(out, ref, f"{name} conn {connectivity} corners {corners_only}")
    assert (t.cpu().numpy() == labels).all()                                  # the input is not written
    print(f"{name}: {ref['edge_count']} edges, {ref['ring_count']} rings, longest {int(ref['rings']['edges'].max(initial=0))}")


# ---- hand-made maps -------------------------------------------------------------------------------------------------------------
def checkerboard(n):
    y, x = np.mgrid[:n, :n]
    return ((y + x) % 2 == 0).astype(np.int32)


def ring_with_island():
    m = np.zeros((20, 23), dtype=np.int32)
    m[2:18, 3:20] = 4
    m[5:15, 6:17] = 0
    m[8:11, 9:13] = 4                            # the same label inside its own hole
    m[9, 10] = 0
    return m


def two_labels():
    m = np.zeros((16, 24), dtype=np.int32)
    m[1:15, 1:12] = 1
    m[1:15, 12:23] = 2                           # a straight shared border ...
    for k in range(6):                           # ... and a staircase
        m[8 + k, 12 - k - 1:12] = 2
    return m


def spiral(n):
    """A one-pixel-wide spiral path: walk inwards, turning right two cells before the path already laid."""
    m = np.zeros((n, n), dtype=np.int32)
    y, x, d = 0, 0, 0
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        dy, dx = step[d]
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ok = 0 <= ny < n and 0 <= nx < n and m[ny, nx] == 0 and not (0 <= ay < n and 0 <= ax < n and m[ay, ax])
        if ok:
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


HAND = {"1x1": np.ones((1, 1)), "1x7": np.ones((1, 7)), "7x1": np.ones((7, 1)), "background": np.zeros((5, 5)),
        "33x65": np.ones((33, 65)), "checkerboard": checkerboard(9), "ring_island": ring_with_island(), "two_labels": two_labels(),
        "spiral": spiral(48)}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_maps(dev, name):
    _check_all(dev, name, HAND[name])


def test_the_hand_made_maps_are_what_they_claim():
    """(no device work) the background map has no ring; the spiral is one ring of a few thousand edges, beyond 2^11: a dozen
    doubling rounds; every interior vertex of the checkerboard is a saddle (one ring under connectivity 8, 41 under 4)."""
    assert outlines_oracle(HAND["background"].astype(np.int32))["ring_count"] == 0
    sp = outlines_oracle(HAND["spiral"].astype(np.int32), 4)
    assert sp["ring_count"] == 1 and 2048 < sp["edge_count"] < 8192
    cb = HAND["checkerboard"]
    assert outlines_oracle(cb, 4)["ring_count"] == 41
    r8 = outlines_oracle(cb, 8)["rings"]
    assert (r8["area2"] > 0).sum() == 1
    ri = outlines_oracle(HAND["ring_island"], 8)["rings"]
    assert (ri["area2"] > 0).sum() == 2 and (ri["area2"] < 0).sum() == 2 and set(ri["label"].tolist()) == {4}


# ---- isolated pixels: the one-work-group scans past their first pass ----------------------------------------------------------------
def _isolated_pixels(H, W):
    """Label 1 where y and x are both odd, and the outlines of that map in closed form: under connectivity 4 every such pixel is
    a region of its own, its ring the unit square from its top-left corner clockwise, led by its top edge 4 * pixel."""
    labels = np.zeros((H, W), dtype=np.int32)
    labels[1::2, 1::2] = 1
    y, x = (a.ravel().astype(np.int32) for a in np.mgrid[1:H:2, 1:W:2])
    n = y.size
    four = np.full(n, 4, dtype=np.int32)
    rings = {"ring": np.arange(n, dtype=np.int32), "label": np.ones(n, dtype=np.int32), "start": 4 * np.arange(n, dtype=np.int32),
             "count": four, "edges": four, "area2": np.full(n, 2, dtype=np.int64), "hole": np.zeros(n, dtype=np.bool_),
             "y0": y, "x0": x, "y1": y + 2, "x1": x + 2, "leader": 4 * (y * W + x)}      # the box is half-open over the vertices
    vertices = np.stack([np.stack([y, x], 1), np.stack([y, x + 1], 1), np.stack([y + 1, x + 1], 1), np.stack([y + 1, x], 1)], 1)
    ref = {"edge_count": 4 * n, "ring_count": n, "vertex_count": 4 * n, "rings": rings,
           "vertices": np.ascontiguousarray(vertices.reshape(-1, 2), dtype=np.int32)}
    return labels, ref


@pytest.mark.parametrize("H,W", [(384, 768), (1056, 1024)])
def test_isolated_pixels_fill_more_than_one_scan_pass(dev, H, W):
    """The array scans of `edges`, `rings` and `write` take 1024 blocks per pass. 384 x 768: 294 912 edges are 1152 blocks of 256
    positions, so the vertex scan runs a second pass and hands its carry to the header's vertex count. 1056 x 1024: 1056 blocks of
    1024 pixels and 1 081 344 edges in 1056 blocks of 1024, so the edge scan and the paired ring scan do too. The capacities are
    exact."""
    import insar_unet_ca_amd as iu
    labels, ref = _isolated_pixels(H, W)
    E, R = ref["edge_count"], ref["ring_count"]
    assert (E + 255) // 256 > 1024 and ((H * W > 1024 * 1024 and E > 1024 * 1024) or H * W < 1024 * 1024)
    out = iu.region_outlines(torch.from_numpy(labels).to(dev), connectivity=4, corners_only=True, max_rings=R, max_vertices=E,
                             max_edges=E)
    _compare(out, ref, f"isolated pixels {H} x {W}")


@pytest.mark.parametrize("W,E", [(32, 1024), (34, 1088)])
def test_rings_end_on_the_numbering_block_boundary(dev, W, E):
    """A distinct label at every even (y, x) of a 32 x W map: one-pixel rings of four edges. 32 x 32 gives E = 1024, exactly one
    numbering block of the count / number kernels, and the last leader's ring ends on its last slot; 32 x 34 gives 1088 and runs
    into a second block."""
    labels = np.zeros((32, W), dtype=np.int32)
    labels[0::2, 0::2] = 1 + np.arange(16 * (W // 2)).reshape(16, W // 2)
    ref = _oracle(f"even pixels 32x{W}", labels, 4, True)
    assert ref["edge_count"] == E and ref["ring_count"] == E // 4 and (ref["rings"]["edges"] == 4).all()
    _check_all(dev, f"even pixels 32x{W}", labels)


# ---- maps labelled by label_regions -------------------------------------------------------------------------------------------------
SPECKLE = {"96x160 at 50 %": (96, 160, 0.5, 11), "70x130 at 30 %": (70, 130, 0.3, 12), "70x130 at 70 %": (70, 130, 0.7, 13)}


def _speckle(H, W, fill, seed):
    """Two classes (1, 2) over a random foreground of the given share."""
    rng = np.random.default_rng(seed)
    return ((rng.random((H, W)) < fill) * rng.integers(1, 3, size=(H, W))).astype(np.uint8)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", list(SPECKLE))
def test_label_regions_maps(dev, case, connectivity):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import outlines as ol
    H, W, fill, seed = SPECKLE[case]
    reg = iu.label_regions(torch.from_numpy(_speckle(H, W, fill, seed)).to(dev), connectivity=connectivity)
    labels = reg["labels"]
    lab = labels.cpu().numpy()
    caps = dict(max_rings=8192, max_vertices=1 << 16, max_edges=1 << 16)
    sc = ol.OutlineScratch(H, W, dev, **caps)
    for corners_only in (True, False):
        ref = _oracle((case, "regions", connectivity), lab, connectivity, corners_only)
        what = f"{case} conn {connectivity} corners {corners_only}"
        first = iu.region_outlines(labels, connectivity=connectivity, corners_only=corners_only, **caps)
        _compare(first, ref, what)
        raw = []
        for _ in range(2):                                                   # a reused scratch: identical bytes, twice
            again = iu.region_outlines(labels, connectivity=connectivity, corners_only=corners_only, scratch=sc, **caps)
            _compare(again, ref, what + " (scratch)")
            raw.append(sc.host.numpy()[:48 * (1 + ref["ring_count"])].tobytes())
            assert torch.equal(first["vertices"], again["vertices"])
        assert raw[0] == raw[1]
        r = first["rings"]
        ids = reg["regions"]["id"]
        area2 = np.zeros(len(ids) + 1, dtype=np.int64)
        np.add.at(area2, r["label"], r["area2"])
        assert (area2[1:] == 2 * reg["regions"]["area"]).all(), what
        per = perimeter_by_label(ref["rings"])
        assert ol.perimeters(r, ids).tolist() == [per[int(i)] for i in ids], what
        assert ((r["area2"] > 0).sum() == reg["count"]) and (np.bincount(r["label"][r["area2"] > 0])[1:] == 1).all()
    if case.startswith("96x160"):
        assert ref["edge_count"] > 8192 and ref["ring_count"] > 256          # more than one block in every scan
    print(f"{case} conn {connectivity}: {ref['edge_count']} edges, {ref['ring_count']} rings, {reg['count']} regions")


# ---- capacities ----------------------------------------------------------------------------------------------------------------------
def test_capacities_and_guards(dev):
    """One below what is needed raises, naming the true count; the bytes after each buffer stay untouched."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd import outlines as ol
    from insar_unet_ca_amd._lib import InsarError, call, ptr
    H, W, fill, seed = SPECKLE["96x160 at 50 %"]
    labels = iu.label_regions(torch.from_numpy(_speckle(H, W, fill, seed)).to(dev), connectivity=8)["labels"]
    ref = _oracle(("96x160 at 50 %", "regions", 8), labels.cpu().numpy(), 8, True)
    E, R, V = ref["edge_count"], ref["ring_count"], ref["vertex_count"]
    exact = iu.region_outlines(labels, max_rings=R, max_vertices=V, max_edges=E)
    _compare(exact, ref, "capacities exactly as needed")
    with pytest.raises(InsarError, match=rf"{E} boundary edges exceed max_edges={E - 1}"):
        iu.region_outlines(labels, max_rings=R, max_vertices=V, max_edges=E - 1)
    with pytest.raises(InsarError, match=rf"{R} rings exceed max_rings={R - 1}"):
        iu.region_outlines(labels, max_rings=R - 1, max_vertices=V, max_edges=E)
    with pytest.raises(InsarError, match=rf"{V} vertices exceed max_vertices={V - 1}"):
        iu.region_outlines(labels, max_rings=R, max_vertices=V - 1, max_edges=E)
    # the phase calls with every buffer inside a guard
    pad = 4096

    def guarded(nbytes):
        g = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=dev)
        return g, g[pad:pad + nbytes]

    def intact(g, nbytes):
        h = g.cpu().numpy()
        return (h[:pad] == 0xA5).all() and (h[pad + nbytes:] == 0xA5).all()

    s = _lib.stream_ptr()
    # edges with one slot too few: E is reported, nothing is written past the scratch or the header
    sb, tb = ol.scratch_bytes(H, W, R, E - 1)
    gs, scratch = guarded(sb)
    gt, table = guarded(tb)
    call("insar_outline_edges", ptr(labels), H, W, 8, E - 1, ptr(scratch), ptr(table), s)
    torch.cuda.synchronize()
    assert int(table.cpu().numpy().view(ol.RING_DTYPE)["edges"][0]) == E
    assert intact(gs, sb) and intact(gt, tb)
    # all five with rings and vertices one too few: the true counts in the header, the first R - 1 / V - 1 as the oracle's
    sb, tb = ol.scratch_bytes(H, W, R - 1, E)
    gs, scratch = guarded(sb)
    gt, table = guarded(tb)
    gv, verts = guarded(8 * (V - 1))
    call("insar_outline_edges", ptr(labels), H, W, 8, E, ptr(scratch), ptr(table), s)
    call("insar_outline_lead", H, W, E, E, ptr(scratch), s)
    call("insar_outline_rank", H, W, E, E, ptr(scratch), s)
    call("insar_outline_rings", ptr(labels), H, W, E, R - 1, E, ptr(scratch), ptr(table), s)
    call("insar_outline_write", H, W, E, 1, R - 1, V - 1, E, ptr(scratch), ptr(table), ptr(verts), s)
    torch.cuda.synchronize()
    assert intact(gs, sb) and intact(gt, tb) and intact(gv, 8 * (V - 1))
    rec = table.cpu().numpy().view(ol.RING_DTYPE)
    assert (int(rec["label"][0]), int(rec["count"][0]), int(rec["edges"][0])) == (R, V, E)
    for f in ("label", "leader", "start", "count", "edges", "area2", "y0", "x0", "y1", "x1"):
        assert (rec[f][1:] == ref["rings"][f][:R - 1]).all(), f
    assert (verts.cpu().numpy().view(np.int32).reshape(-1, 2) == ref["vertices"][:V - 1]).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_detect_with_outlines(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    scene = np.random.default_rng(4).standard_normal((64, 96)).astype(np.float32)
    pred = iu.ScenePredictor(net, tile=32, overlap=8, batch=4, num_classes=2)
    # an untrained net puts every pixel in one class: move the output bias by the median log-odds, so that the class map
    # splits about evenly and falls into many regions
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():
        net.outc.bias[1] += torch.log(p[0] / p[1]).median()
    for connectivity in (8, 4):
        kw = dict(connectivity=connectivity, min_area=2)
        plain = pred.detect(scene, **kw)
        det = pred.detect(scene, outlines=True, **kw)
        assert "outlines" not in plain and "perimeter" not in plain["regions"]
        for k in ("mask", "conf", "labels", "mask_clean"):
            assert torch.equal(plain[k], det[k]), k
        assert plain["count"] == det["count"] and set(det["regions"]) == set(plain["regions"]) | {"perimeter"}
        for k, v in plain["regions"].items():
            assert v.tobytes() == det["regions"][k].tobytes(), k
        direct = iu.region_outlines(det["labels"], connectivity=connectivity)
        o = det["outlines"]
        assert torch.equal(o["vertices"], direct["vertices"])
        assert all(o[k] == direct[k] for k in ("ring_count", "vertex_count", "edge_count"))
        for f, v in direct["rings"].items():
            assert v.tobytes() == o["rings"][f].tobytes(), f
        lab = det["labels"].cpu().numpy()
        ref = outlines_oracle(lab, connectivity)
        _compare(o, ref, f"detect conn {connectivity}")
        per = perimeter_by_label(ref["rings"])
        assert det["regions"]["perimeter"].tolist() == [per[int(i)] for i in det["regions"]["id"]]
        back = np.zeros_like(lab)
        for e in iu.to_polygons(o):
            rings = [r for p in e["polygons"] for r in [p["exterior"]] + p["holes"]]
            inside = rasterise(rings, *lab.shape)
            assert (back[inside] == 0).all()
            back[inside] = e["label"]
        assert (back == lab).all()
    one = iu.detect_scene(net, scene, outlines=True, tile=32, overlap=8, batch=4, num_classes=2, connectivity=4, min_area=2)
    assert torch.equal(one["outlines"]["vertices"], det["outlines"]["vertices"])
    print(f"detect: {det['count']} regions, {o['ring_count']} rings, {o['vertex_count']} vertices")
    assert det["count"] > 4 and o["ring_count"] >= det["count"]
