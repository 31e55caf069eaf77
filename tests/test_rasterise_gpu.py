"""GPU: polygon rasterisation (insar_unet_ca_amd/rasterise.py on csrc/raster.hip) against the restatement of
tests/rasterise_ref.py (pinned by tests/test_rasterise_host.py).

Every comparison is bitwise, for uint8 and int32, and the device's overlap count equals the restatement's. The shapes are the
smallest that cross each boundary of the kernels: widths that are no multiple of 4 (scalar tails) and of 256 (a wave's
chunk), heights that are no multiple of the band, both sides of every width at which the rows per band change (queried from
the library), the widest legal scene (one row per band, all 16 waves on one row), an edge that crosses more than 64 rows (the
wave shares it) and a band whose record list is far longer than a work-group."""
import numpy as np
import pytest
import torch

from tests import rasterise_ref as ref
from tests.test_rasterise_host import AFFINE, _poly, random_scene, speckle, star

pytestmark = pytest.mark.gpu
NP = {torch.uint8: np.uint8, torch.int32: np.int32}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _check(dev, table, H, W, what, dtypes=(torch.uint8, torch.int32), base=None, **kw):
    """Both element types bitwise against the restatement; returns the int32 (or last) map."""
    import insar_unet_ca_amd as iu
    cover, vsum = ref.cover_vsum(table.edges, H, W)
    edges_before = table.edges.copy()
    for dt in dtypes:
        b = None if base is None else torch.from_numpy(base.astype(NP[dt])).to(dev)
        want, void = ref.decide(cover, vsum, NP[dt], base=None if base is None else base.astype(NP[dt]), **kw)
        out = iu.rasterise_polygons(table, H, W, dtype=dt, base=b, device=dev, **kw)
        got = out["labels"].cpu().numpy()
        assert out["labels"].dtype == dt and got.shape == (H, W) and out["overlap_pixels"].dtype == torch.int64
        bad = np.argwhere(got != want)
        print(f"{what} {dt}: {len(table)} edges, {table.crossings(H)} crossings, {void} void, {len(bad)} pixels differ")
        assert got.tobytes() == want.tobytes(), f"{what} {dt}: differs at {bad[:8].tolist()}"
        assert int(out["overlap_pixels"]) == void, f"{what} {dt}: overlap_pixels {int(out['overlap_pixels'])}, restatement {void}"
        if b is not None:
            assert b.cpu().numpy().tobytes() == base.astype(NP[dt]).tobytes()              # the base map is not written
    assert table.edges.tobytes() == edges_before.tobytes()
    assert table.device_edges(dev).cpu().numpy().tobytes() == edges_before.tobytes() or len(table) == 0
    return got


def scene_for(H, W, seed, n_poly=4):
    """Stars with holes scaled to an H x W map (some vertices outside), labels 1, 2, ... and one above 255."""
    import insar_unet_ca_amd as iu
    rng = np.random.default_rng(seed)
    polys = []
    for k in range(n_poly):
        cy, cx = rng.uniform(-0.1, 1.1) * H, rng.uniform(-0.1, 1.1) * W
        ring = star(rng, 0, 0, 0.5, 1.0, int(rng.integers(3, 9)))
        sy, sx = rng.uniform(0.3, 0.8) * H + 1, rng.uniform(0.3, 0.8) * W + 1
        ext = np.rint((ring * (sy, sx) + (cy, cx)) * 256) / 256
        holes = [np.rint((ring * (0.4 * sy, 0.4 * sx) + (cy, cx)) * 256) / 256] if k % 2 == 0 else []
        polys.append({"label": 300 if k == 3 else k + 1, "polygons": [{"exterior": ext, "holes": holes}]})
    return iu.pack_polygons(polys)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (37, 53), (5, 260), (70, 12)])
def test_small_and_odd_shapes(dev, shape):
    H, W = shape
    _check(dev, scene_for(H, W, seed=H * 100 + W), H, W, f"{H}x{W}")


def test_more_bands_than_one_scan_pass(dev):
    """32 800 x 8 is 1025 bands of 32 rows, and the scan of the band counters takes 1024 per pass: the last band gets its slice of
    the record array from the carry of the first pass. Two rectangles, one through every band and one inside the last."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import rasterise as rs
    H, W = 32800, 8
    assert rs.band_rows(W) == 32
    rect = lambda y0, x0, y1, x1: np.array([[y0, x0], [y0, x1], [y1, x1], [y1, x0]], dtype=np.float64)
    table = iu.pack_polygons([{"label": 7, "polygons": [{"exterior": rect(3, 1, H - 40, 4), "holes": []}]},
                              {"label": 9, "polygons": [{"exterior": rect(H - 20, 2, H - 2, 7), "holes": []}]}])
    want = np.zeros((H, W), dtype=np.int32)
    want[3:H - 40, 1:4] = 7
    want[H - 20:H - 2, 2:7] = 9
    for dt in (torch.uint8, torch.int32):
        out = iu.rasterise_polygons(table, H, W, dtype=dt, device=dev)
        assert np.array_equal(out["labels"].cpu().numpy(), want.astype(NP[dt])) and int(out["overlap_pixels"]) == 0


def _band_boundaries():
    from insar_unet_ca_amd import rasterise as rs
    rows = [rs.band_rows(W) for W in range(1, 16385)]
    return [W for W in range(1, 16384) if rows[W - 1] != rows[W]]                         # W and W + 1 differ


def test_band_rows_change_where_expected():
    from insar_unet_ca_amd import rasterise as rs
    b = _band_boundaries()
    assert len(b) == 5 and [rs.band_rows(W) for W in b] == [32, 16, 8, 4, 2] and rs.band_rows(16384) == 1


@pytest.mark.parametrize("k", range(5))
def test_both_sides_of_every_band_boundary(dev, k):
    from insar_unet_ca_amd import rasterise as rs
    for W in (_band_boundaries()[k], _band_boundaries()[k] + 1):
        H = 2 * rs.band_rows(W) + 1
        _check(dev, scene_for(H, W, seed=W), H, W, f"band boundary {H}x{W} (R = {rs.band_rows(W)})")


def test_widest_scene(dev):
    import insar_unet_ca_amd as iu
    table = scene_for(3, 16384, seed=3)
    _check(dev, table, 3, 16384, "3x16384")
    with pytest.raises(iu.InsarError, match="16384"):
        iu.rasterise_polygons(table, 3, 16385, device=dev)


def test_odd_width_int32_with_a_misaligned_base(dev):
    """W % 4 != 0 takes the guarded scalar path; with W % 4 == 0 a base 4 bytes off a 16-byte boundary is read by scalars while
    the output is stored 16 bytes at a time. Slices are accepted: misalignment is no error."""
    import insar_unet_ca_amd as iu
    for H, W in ((9, 31), (9, 32)):
        table = scene_for(H, W, seed=77)
        flat = torch.arange(H * W + 4, dtype=torch.int32, device=dev) % 11 + 1000
        base = flat[1:1 + H * W].view(H, W)
        assert base.data_ptr() % 16 == 4 and base.is_contiguous()
        want, void = ref.rasterise(table.edges, H, W, np.int32, fill=5, base=base.cpu().numpy())
        out = iu.rasterise_polygons(table, H, W, dtype=torch.int32, fill=5, base=base)
        assert out["labels"].cpu().numpy().tobytes() == want.tobytes() and int(out["overlap_pixels"]) == void
        assert (flat.cpu().numpy() == np.arange(H * W + 4) % 11 + 1000).all()
        b8 = (torch.arange(H * W + 4, device=dev) % 200).to(torch.uint8)[1:1 + H * W].view(H, W)
        want, void = ref.rasterise(table.edges, H, W, np.uint8, base=b8.cpu().numpy())
        out = iu.rasterise_polygons(table, H, W, base=b8)
        assert out["labels"].cpu().numpy().tobytes() == want.tobytes() and int(out["overlap_pixels"]) == void


def test_vertices_beyond_all_four_sides(dev):
    import insar_unet_ca_amd as iu
    H, W = 40, 70
    ring = [(-10.25, 35), (20, 90.5), (55.125, 30), (18, -20.75)]
    table = iu.pack_polygons([_poly(ring, 9, holes=[[(10, 20), (10, 50), (30, 50), (30, 20)]])])
    got = _check(dev, table, H, W, "beyond all sides")
    assert got[0, 35] == 9 and got[20, 35] == 0 and got[0, 0] == 0 and got[39, 69] == 0 and got[39, 30] == 9
    far = iu.pack_polygons([_poly([(-65536, -65536), (-65536, 65536), (65536, 65536), (65536, -65536)], 4)])   # the coordinate limit
    assert (_check(dev, far, H, W, "far corners") == 4).all()


def test_an_edge_spanning_every_row(dev):
    """Edges of 300 rows: each is shared out over the lanes of a wave, 64 rows at a time, across ten 32-row bands."""
    import insar_unet_ca_amd as iu
    H, W = 300, 45
    table = iu.pack_polygons([_poly([(-3, 2.3), (-2, 40.7), (310, 30.2), (305, 11.1)], 2), _poly([(0, 20), (300, 25), (300, 20)], 3)])
    got = _check(dev, table, H, W, "tall edges")
    assert (got == 255).any() and (got == 2).any()
    H, W = 200, 8800                                                                       # one row per band: 200 bands per edge
    _check(dev, iu.pack_polygons([_poly([(-1, 10.5), (-1, 8000.25), (201, 8790), (201, 300)], 6)]), H, W, "tall edges, R = 1",
           dtypes=(torch.uint8,))


def test_two_thousand_slivers_through_one_row(dev):
    import insar_unet_ca_amd as iu
    H, W = 5, 1000
    x = np.arange(2000) * 0.5
    slivers = [_poly([(1.25, a), (1.25, a + 0.25), (3.75, a + 0.375), (3.75, a + 0.125)], 1 + i % 3) for i, a in enumerate(x)]
    table = iu.pack_polygons(slivers)
    assert table.crossings(H) >= 3 * 4000 - 4000
    _check(dev, table, H, W, "slivers")


def test_empty_table_and_edges_all_outside(dev):
    import insar_unet_ca_amd as iu
    H, W = 33, 47
    empty = iu.pack_polygons([])
    assert len(empty) == 0 and empty.bounds is None
    base = (np.arange(H * W).reshape(H, W) % 5).astype(np.int32)
    assert (_check(dev, empty, H, W, "empty", fill=3) == 3).all()
    _check(dev, empty, H, W, "empty over a base", base=base)
    outside = iu.pack_polygons([_poly([(-20, 3), (-20, 30), (-5, 30), (-5, 3)], 1), _poly([(40, 3), (40, 30), (90, 17)], 2),
                                _poly([(2, 50), (2, 90), (30, 90), (30, 50)], 3)])         # above, below, to the right
    assert outside.crossings(H) == 2 * 28
    assert (_check(dev, outside, H, W, "all outside", fill=7) == 7).all()
    left = iu.pack_polygons([_poly([(2, -50), (2, -9), (30, -9), (30, -50)], 3)])           # to the left: +1 - 1 at column 0
    assert (_check(dev, left, H, W, "left of the scene") == 0).all()


@pytest.mark.parametrize("seed", range(3))
def test_random_overlaps(dev, seed):
    import insar_unet_ca_amd as iu
    H, W = 61, 83
    table = iu.pack_polygons(random_scene(np.random.default_rng(300 + seed), H, W, n_poly=7))
    got = _check(dev, table, H, W, f"overlaps {seed}")
    assert (got == 255).sum() > 0


def test_holes_fill_overlap_value_and_base(dev):
    import insar_unet_ca_amd as iu
    H, W = 50, 66
    nested = _poly([(2, 2), (2, 60), (46, 60), (46, 2)], 1, holes=[[(8, 8), (8, 30.5), (40, 30.5), (40, 8)], [(8.5, 35), (20, 50), (40, 33.25)]])
    island = _poly([(12, 12), (12, 25), (30, 25), (30, 12)], 2)                             # inside the first hole
    clash = _poly([(30, 40), (30, 64), (49, 64), (49, 40)], 3)                              # over the exterior: void
    table = iu.pack_polygons([nested, island, clash])
    got = _check(dev, table, H, W, "holes")
    assert got[9, 9] == 0 and got[13, 13] == 2 and got[3, 3] == 1 and got[45, 59] == 255 and got[48, 63] == 3
    base = (np.arange(H * W).reshape(H, W) % 13 + 20).astype(np.int32)
    got = _check(dev, table, H, W, "holes, fill 9, void 77", fill=9, overlap_value=77)
    assert got[9, 9] == 9 and got[45, 59] == 77
    got = _check(dev, table, H, W, "holes over a base, void 2", base=base, overlap_value=2)
    assert got[9, 9] == base[9, 9] and got[13, 13] == 2 and got[0, 0] == base[0, 0]


def blobs(rng, H, W):
    y, x = np.mgrid[:H, :W]
    m = np.zeros((H, W), dtype=bool)
    for _ in range(9):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(4, 14)
        m ^= (y - cy) ** 2 + (x - cx) ** 2 < r * r                                           # xor: rings and holes
    return m


@pytest.mark.parametrize("kind,shape", [("speckle", (64, 96)), ("blobs", (96, 160))])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_round_trip_on_the_device(dev, kind, shape, connectivity):
    import insar_unet_ca_amd as iu
    H, W = shape
    rng = np.random.default_rng(H + connectivity)
    mask = (speckle(rng, H, W) > 0) if kind == "speckle" else blobs(rng, H, W)
    labels = iu.label_regions(torch.from_numpy(mask.astype(np.uint8)).to(dev), connectivity=connectivity)["labels"]
    outl = iu.region_outlines(labels, connectivity=connectivity, max_rings=8192, max_vertices=1 << 17, max_edges=1 << 17)
    want = labels.cpu().numpy()
    plain = iu.pack_polygons(iu.to_polygons(outl))
    out = iu.rasterise_polygons(plain, H, W, dtype=torch.int32, device=dev)
    assert out["labels"].cpu().numpy().tobytes() == want.tobytes() and int(out["overlap_pixels"]) == 0
    world = iu.pack_polygons(iu.to_polygons(outl, transform=AFFINE), transform=AFFINE)
    assert world.edges.tobytes() == plain.edges.tobytes()
    fc = iu.to_geojson(outl, transform=AFFINE)
    back = iu.labels_from_geojson(fc, H, W, transform=AFFINE, dtype=torch.int32, device=dev)
    assert back.cpu().numpy().tobytes() == want.tobytes()
    print(f"{kind} {H}x{W} conn {connectivity}: {int(want.max())} regions, {len(plain)} edges")


def test_determinism_and_scratch_reuse(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import rasterise as rs
    H, W = 61, 83
    table = iu.pack_polygons(random_scene(np.random.default_rng(42), H, W, n_poly=9))
    base = torch.arange(H * W, device=dev).remainder(7).to(torch.uint8).view(H, W)
    keep = base.clone()
    scratch = iu.RasterScratch(H, W, dev, table.crossings(H) + 100)
    runs = [iu.rasterise_polygons(table, H, W, base=base) for _ in range(2)]
    runs += [iu.rasterise_polygons(table, H, W, base=base, scratch=scratch) for _ in range(3)]
    other = iu.pack_polygons(random_scene(np.random.default_rng(43), H, W, n_poly=2))
    iu.rasterise_polygons(other, H, W, scratch=scratch)                                     # another table through the scratch
    runs.append(iu.rasterise_polygons(table, H, W, base=base, scratch=scratch))
    first = runs[0]["labels"].cpu().numpy().tobytes()
    assert all(r["labels"].cpu().numpy().tobytes() == first and int(r["overlap_pixels"]) == int(runs[0]["overlap_pixels"]) for r in runs)
    assert torch.equal(base, keep) and rs.launches() == 5
    with pytest.raises(iu.InsarError, match="scratch"):
        iu.rasterise_polygons(table, H, W, scratch=iu.RasterScratch(H, W, dev, 3))
    with pytest.raises(iu.InsarError, match="scratch"):
        iu.rasterise_polygons(table, H, W + 1, scratch=scratch)


def test_feeds_crop_index_and_region_overlaps(dev):
    import insar_unet_ca_amd as iu
    H = W = 64
    fc = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {"label": 1, "site": "a"}, "geometry": {"type": "Polygon", "coordinates": [
            [[4, 4], [40.5, 6], [38, 30.25], [6, 28]], [[10, 10], [20, 10], [20, 20], [10, 20]]]}},
        {"type": "Feature", "properties": {"label": 1, "site": "b"}, "geometry": {"type": "MultiPolygon", "coordinates": [
            [[[44, 44], [60, 44], [60, 60], [44, 60], [44, 44]]], [[[2, 50], [12, 50], [7, 62]]]]}}]}
    gt = iu.labels_from_geojson(fc, H, W, device=dev)
    assert gt.dtype == torch.uint8 and tuple(gt.shape) == (H, W)
    want, _ = ref.rasterise(iu.from_geojson(fc).edges, H, W)
    assert gt.cpu().numpy().tobytes() == want.tobytes() and set(np.unique(want)) == {0, 1}
    idx = iu.CropIndex(gt, num_classes=2, cell=8)
    assert int(idx.class_pixels()[1]) == int((want == 1).sum())
    inst = iu.labels_from_geojson(fc, H, W, device=dev, dtype=torch.int32, value_property="site", values={"a": 1, "b": 2})
    pred = iu.label_regions(gt, connectivity=8)["labels"]
    p, g, n = iu.region_overlaps(pred, inst)
    assert int(np.asarray(n).sum()) == int((want == 1).sum()) and set(np.asarray(g).tolist()) == {1, 2}
