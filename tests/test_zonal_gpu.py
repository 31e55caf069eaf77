"""GPU: per-region statistics of a raster (insar_unet_ca_amd/zonal.py on csrc/zonal.hip) against the numpy restatement of
tests/zonal_ref.py (pinned against a pixel loop in tests/test_zonal_host.py).

Every comparison of an integer field is exact; the float fields to 1e-12 relative (the same integers divided in float64 on
both sides). The map is 200 x 264 unless a case says otherwise: ragged against the four pixels of a thread, the 64 lanes of
a wave and the 1024 pixels of a work-group pass; 52 800 pixels are 52 passes, so a small `max_regions` meets several
work-groups and several changes of the label a work-group keeps in LDS."""
import numpy as np
import pytest
import torch

from tests import zonal_ref as ref

pytestmark = pytest.mark.gpu
H0, W0 = 200, 264
I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _compare(got, want, what=""):
    fields = ref.INT_FIELDS + (ref.HIST_FIELDS if want["bins"] else ())
    assert ("hist" in got) == bool(want["bins"]) and ("below" in got) == bool(want["bins"])
    for f in fields:
        assert got[f].shape == want[f].shape, f"{what}: {f} {got[f].shape} {want[f].shape}"
        bad = np.flatnonzero(np.asarray(got[f] != want[f]).reshape(-1))
        assert bad.size == 0, f"{what}: {f} differs at {bad[:5]}: {got[f].reshape(-1)[bad[:5]]} vs {want[f].reshape(-1)[bad[:5]]}"
    assert got["sumsq_q"].dtype == object and got["argmin"].dtype == np.int32 and got["n"].dtype == np.int64
    assert got["out_of_range"] == want["out_of_range"], what
    assert got["range_q"] == want["range_q"] and got["scale"] == want["scale"]
    for f in ref.FLOAT_FIELDS:
        assert got[f].dtype == np.float64
        assert (np.isnan(got[f]) == (want["n"] == 0)).all(), f"{what}: {f} NaN pattern"
        np.testing.assert_allclose(got[f], want[f], rtol=1e-12, atol=0, err_msg=f"{what}: {f}")
    if want["bins"]:
        assert ((got["hist"].sum(axis=-1) + got["below"] + got["above"]) == got["n"]).all(), what


def _check(dev, labels, raster, what="", **kw):
    import insar_unet_ca_amd as iu
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    raster = np.ascontiguousarray(raster)
    l, r = torch.from_numpy(labels).to(dev), torch.from_numpy(raster).to(dev)
    got = iu.region_stats(l, r, **kw)
    want = ref.region_stats_ref(labels, raster, **kw)
    _compare(got, want, what)
    # the inputs are not written
    assert np.array_equal(l.cpu().numpy(), labels) and np.array_equal(r.cpu().numpy().view(np.uint8), raster.view(np.uint8)), what
    print(f"{what}: {int((want['n'] > 0).sum())} regions with pixels, n up to {int(want['n'].max(initial=0))}, "
          f"{int(want['n_invalid'].sum())} invalid, {int(want['n_clipped'].sum())} clipped, {want['out_of_range']} out of range")
    return got, want


def patches(H, W, seed, nlab=40, size=23):
    """Random rectangular patches of random ids over background; ids 3, 17 and nlab are never used."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), dtype=np.int32)
    ids = [i for i in range(1, nlab) if i not in (3, 17)]
    for _ in range(150):
        y, x = rng.integers(0, H), rng.integers(0, W)
        lab[y:y + rng.integers(1, size), x:x + rng.integers(1, size)] = ids[rng.integers(0, len(ids))]
    return lab


def dirty_normal(H, W, seed, nodata=-9999.0):
    rng = np.random.default_rng(seed)
    r = rng.normal(size=(H, W)).astype(np.float32)
    pos = rng.choice(H * W, size=1500, replace=False)
    r.ravel()[pos] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, nodata], dtype=np.float32), pos.size)
    return r


# ---- all fields ----------------------------------------------------------------------------------------------------------
def test_random_patches_with_invalid_pixels(dev):
    lab, r = patches(H0, W0, 1), dirty_normal(H0, W0, 2)
    got, want = _check(dev, lab, r, "patches", max_regions=40, nodata=-9999.0)
    assert want["n_invalid"].sum() > 100 and (want["n"][[2, 16, 39]] == 0).all() and (want["n_invalid"][[2, 16, 39]] == 0).all()
    _check(dev, lab, r, "patches, no nodata", max_regions=40)                       # -9999 * 2^16 is inside the clamp
    got, want = _check(dev, lab, r, "patches, count", max_regions=64, count=20)
    assert got["n"].shape == (20,)
    _check(dev, lab, r, "patches, default table")                                   # 65536 records, most of them untouched


def test_one_region_where_every_pixel_clips(dev):
    """+-4e4 at scale 2^16 is +-2.6e9: every q is +-(2^31 - 1), the square sum 52 800 * (2^31 - 1)^2 ~ 2^77.7. Every wave of every
    work-group meets one record: the LDS fold and the split square sum."""
    rng = np.random.default_rng(3)
    r = (np.where(rng.random((H0, W0)) < 0.5, -4e4, 4e4) + rng.normal(size=(H0, W0))).astype(np.float32)
    lab = np.ones((H0, W0), dtype=np.int32)
    got, want = _check(dev, lab, r, "one region", max_regions=1)
    assert got["n_clipped"][0] == got["n"][0] == H0 * W0
    assert got["sumsq_q"][0] == H0 * W0 * ref.Q_LIMIT ** 2 > 1 << 77
    assert got["min_q"][0] == -ref.Q_LIMIT and got["max_q"][0] == ref.Q_LIMIT
    _check(dev, lab, r, "one region, unclipped", max_regions=1, scale=1.0)


def test_labels_alternating_per_pixel(dev):
    lab = (1 + (np.arange(H0 * W0) % 2)).reshape(H0, W0).astype(np.int32)
    _check(dev, lab, dirty_normal(H0, W0, 4), "alternating", max_regions=2, nodata=-9999.0)
    lab3 = (1 + (np.arange(H0 * W0) % 3)).reshape(H0, W0).astype(np.int32)          # every run one pixel, no period of 4
    _check(dev, lab3, dirty_normal(H0, W0, 5), "period 3", max_regions=3)


@pytest.mark.parametrize("width", [5, 64])
def test_vertical_stripes(dev, width):
    lab = (1 + ((np.arange(W0) + 3) // width)).astype(np.int32)[None, :].repeat(H0, axis=0)
    _check(dev, lab, dirty_normal(H0, W0, 6), f"stripes {width}", max_regions=int(lab.max()), nodata=-9999.0, bins=16, range=(-2.0, 2.0))


def test_label_bounds_and_the_bytes_around_the_table(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import zonal
    R = 12
    rng = np.random.default_rng(7)
    lab = rng.integers(-3, R + 1, size=(H0, W0)).astype(np.int32)
    lab[5, :40] = R + 1
    lab[9, 100:130] = I32_MAX
    lab[11, 3:9] = I32_MIN
    lab[13, :50] = R
    r = rng.normal(size=(H0, W0)).astype(np.float32)
    want = ref.region_stats_ref(lab, r, max_regions=R, bins=7, range=(-1.0, 1.0))
    assert want["out_of_range"] == 70 and want["n"][R - 1] > 50
    tb = zonal.scratch_bytes(R, 7, 1)
    guard = 4096
    big = torch.full((tb + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    sc = zonal.ZonalScratch(dev, R, 7, 1, table=big[guard:guard + tb])
    l, rr = torch.from_numpy(lab).to(dev), torch.from_numpy(r).to(dev)
    got = iu.region_stats(l, rr, max_regions=R, bins=7, range=(-1.0, 1.0), scratch=sc)
    _compare(got, want, "bounds")
    host = big.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + tb:] == 0xA5).all()
    assert np.array_equal(host[guard:guard + tb], sc.host.numpy())


# ---- ties ----------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_first_pixel(dev):
    lab = patches(H0, W0, 8)
    got, want = _check(dev, lab, np.full((H0, W0), 2.5, dtype=np.float32), "constant", max_regions=40)
    for i in np.flatnonzero(want["n"] > 0):
        first = np.flatnonzero(lab.ravel() == i + 1)[0]
        assert tuple(got["argmin"][i]) == tuple(got["argmax"][i]) == (first // W0, first % W0)
    # two equal peaks and two equal troughs in one region: the earlier one; a second region whose only valid pixel is its last
    lab = np.zeros((H0, W0), dtype=np.int32)
    lab[10:150, 20:250] = 1
    lab[160:190, 7:201] = 2
    r = np.random.default_rng(9).random((H0, W0)).astype(np.float32)
    r[140, 30] = r[20, 240] = 5.0
    r[149, 249] = r[30, 21] = -5.0
    r[lab == 2] = np.nan
    r[189, 200] = 0.25
    got, want = _check(dev, lab, r, "peaks", max_regions=2)
    assert tuple(got["argmax"][0]) == (20, 240) and tuple(got["argmin"][0]) == (30, 21)
    assert got["n"][1] == 1 and tuple(got["argmin"][1]) == tuple(got["argmax"][1]) == (189, 200) and got["min_q"][1] == 16384


# ---- element types -------------------------------------------------------------------------------------------------------
def test_uint8_raster(dev):
    lab = patches(H0, W0, 10)
    r = np.random.default_rng(11).integers(0, 256, size=(H0, W0), dtype=np.uint8)
    got, want = _check(dev, lab, r, "uint8", max_regions=40, nodata=255, bins=256, range=(0, 256))
    assert want["n_invalid"].sum() > 0 and got["scale"] == 1.0
    _check(dev, lab, r, "uint8 plain", max_regions=40)
    _check(dev, lab[:, :263], r[:, :263], "uint8 odd width", max_regions=40)        # no 4-byte loads


def test_int32_raster_with_the_extreme_values(dev):
    from insar_unet_ca_amd import zonal
    import insar_unet_ca_amd as iu
    lab = patches(H0, W0, 12, nlab=10, size=60)
    r = np.random.default_rng(13).integers(-10 ** 6, 10 ** 6, size=(H0, W0)).astype(np.int32)
    ys, xs = np.nonzero(lab == 1)
    r[ys[3], xs[3]], r[ys[-2], xs[-2]] = I32_MIN, I32_MAX
    r[ys[0], xs[0]] = I32_MAX                                      # an earlier maximum
    ys, xs = np.nonzero(lab == 2)
    r[ys, xs] = I32_MIN                                            # q^2 = 2^62 on every pixel
    got, want = _check(dev, lab, r, "int32", max_regions=10)
    assert (got["n_clipped"] == 0).all() and got["min_q"][0] == I32_MIN and got["max_q"][0] == I32_MAX
    assert got["sumsq_q"][1] == int(want["n"][1]) << 62
    sc = zonal.ZonalScratch(dev, 10, 0, 1)
    iu.region_stats(torch.from_numpy(lab).to(dev), torch.from_numpy(r).to(dev), max_regions=10, scratch=sc)
    rec = sc.host.numpy().view(zonal.ZONAL_DTYPE)
    i0, i1 = int(np.flatnonzero((lab == 1).ravel())[3]), int(np.flatnonzero((lab == 1).ravel())[0])
    assert int(rec["min_key"][1]) == (0 << 32) | i0                                 # INT32_MIN biased is 0
    assert int(rec["max_key"][1]) == (0xFFFFFFFF << 32) | (0xFFFFFFFF & ~i1)
    _check(dev, lab, r, "int32 nodata", max_regions=10, nodata=I32_MIN, bins=5, range=(-10 ** 6, 10 ** 6))


def test_largest_inscribed_radius_from_the_distance_transform(dev):
    """max of the d2 map of `distance_transform` (distance to the nearest pixel that is not of the region) per region = the
    brute-force largest inscribed radius squared."""
    import insar_unet_ca_amd as iu
    H, W = 60, 90
    lab = np.zeros((H, W), dtype=np.int32)
    yy, xx = np.mgrid[:H, :W]
    lab[(yy - 20) ** 2 + (xx - 25) ** 2 <= 14 ** 2] = 1
    lab[35:55, 50:85] = 2
    lab[5:8, 60:80] = 3
    l = torch.from_numpy(lab).to(dev)
    d2 = iu.distance_transform(l, sites=("eq", 0), max_distance=None)["d2"]
    assert d2.dtype == torch.int32 and tuple(d2.shape[-2:]) == (H, W)
    got = iu.region_stats(l, d2.reshape(H, W).contiguous(), max_regions=3)
    by, bx = np.nonzero(lab == 0)
    for k in (1, 2, 3):
        ys, xs = np.nonzero(lab == k)
        best = max(int(((by - y) ** 2 + (bx - x) ** 2).min()) for y, x in zip(ys, xs))
        assert got["max_q"][k - 1] == best and got["max"][k - 1] == float(best), k
    assert got["min_q"].tolist() == [1, 1, 1]


# ---- histogram -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 7, 256])
def test_histogram_with_values_on_every_edge(dev, bins):
    lab = patches(H0, W0, 14)
    rng = np.random.default_rng(15)
    q_lo, q_hi = -1000, 1001                                      # a width no bin count here divides
    edges = np.array([q_lo + -(-b * (q_hi - q_lo) // bins) for b in range(bins)] + [q_lo, q_hi, q_lo - 1, q_hi - 1, q_hi + 1])
    vals = rng.integers(q_lo - 300, q_hi + 300, size=(H0, W0))
    vals.ravel()[rng.choice(H0 * W0, size=8 * edges.size, replace=False)] = np.tile(edges, 8)
    vals.ravel()[rng.choice(H0 * W0, size=8 * edges.size, replace=False)] = np.tile(edges - 1, 8)
    got, want = _check(dev, lab, vals.astype(np.int32), f"int edges / {bins}", max_regions=40, bins=bins, range=(q_lo, q_hi))
    assert want["below"].sum() > 0 and want["above"].sum() > 0
    # the same through the float path: q = v * 2 exactly, the range goes through the same quantisation
    _check(dev, lab, vals.astype(np.float32), f"float edges / {bins}", max_regions=40, scale=2.0, bins=bins, range=(q_lo, q_hi))
    # the widest range there is: every in-range product (q - q_lo) * bins stays exact
    wide = rng.integers(I32_MIN, I32_MAX, size=(H0, W0), endpoint=True).astype(np.int32)
    _check(dev, lab, wide, f"full range / {bins}", max_regions=40, bins=bins, range=(I32_MIN, I32_MAX))


def test_percentile_of_device_histograms(dev):
    import insar_unet_ca_amd as iu
    lab = patches(H0, W0, 16)
    r = np.random.default_rng(17).random((H0, W0)).astype(np.float32)
    got, _ = _check(dev, lab, r, "percentile", max_regions=40, bins=64, range=(0.0, 1.0))
    med = iu.percentile(got, 50)
    for i in np.flatnonzero(got["n"] > 50):
        assert abs(med[i] - np.median(r[lab == i + 1])) <= 1.5 / 64 + 0.5 / np.sqrt(got["n"][i])
    assert np.isnan(med[2])


# ---- channels, shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_multi_channel_equals_single_channel_calls(dev, dtype):
    import insar_unet_ca_amd as iu
    lab = patches(H0, W0, 18)
    if dtype == np.float32:
        r = np.stack([dirty_normal(H0, W0, 19 + c) * (10.0 ** c) for c in range(3)])
        kw = dict(max_regions=40, nodata=-9999.0, bins=9, range=(-3.0, 3.0))
    else:
        r = np.random.default_rng(20).integers(0, 256, size=(3, H0, W0), dtype=np.uint8)
        kw = dict(max_regions=40, bins=9, range=(3, 250))
    got, want = _check(dev, lab, r, "three channels", **kw)
    assert got["n"].shape == (3, 40) and got["argmin"].shape == (3, 40, 2) and got["hist"].shape == (3, 40, 9)
    l = torch.from_numpy(lab).to(dev)
    for c in range(3):
        one = iu.region_stats(l, torch.from_numpy(r[c]).to(dev), **kw)
        for f in ref.INT_FIELDS + ref.HIST_FIELDS + ref.FLOAT_FIELDS:
            if f == "sumsq_q":
                assert (one[f] == got[f][c]).all()
            else:
                assert one[f].tobytes() == got[f][c].tobytes(), (c, f)
    four = np.concatenate([r, r[:1]])
    _check(dev, lab, four, "four channels", **kw)


@pytest.mark.parametrize("H, W", [(1, 1), (1, 7), (3, 5), (37, 61)])
def test_small_shapes(dev, H, W):
    rng = np.random.default_rng(21)
    lab = rng.integers(0, 4, size=(H, W)).astype(np.int32)
    lab[0, 0] = 1
    _check(dev, lab, rng.normal(size=(H, W)).astype(np.float32), f"{H}x{W}", max_regions=3, bins=4, range=(-1.0, 1.0))
    _check(dev, lab, rng.integers(0, 256, size=(H, W), dtype=np.uint8), f"{H}x{W} uint8", max_regions=3)
    _check(dev, lab, rng.integers(-9, 9, size=(2, H, W)).astype(np.int32), f"{H}x{W} int32", max_regions=2)


def test_views_off_every_vector_boundary(dev):
    """Contiguous views that start 4 and 1 bytes into an allocation: guarded scalar loads, the same result."""
    import insar_unet_ca_amd as iu
    lab, r = patches(H0, W0, 22), dirty_normal(H0, W0, 23)
    u8 = np.random.default_rng(24).integers(0, 256, size=(H0, W0), dtype=np.uint8)
    lb = torch.zeros(H0 * W0 + 1, dtype=torch.int32, device=dev)
    rb = torch.zeros(H0 * W0 + 1, dtype=torch.float32, device=dev)
    ub = torch.zeros(H0 * W0 + 1, dtype=torch.uint8, device=dev)
    lv, rv, uv = lb[1:].view(H0, W0), rb[1:].view(H0, W0), ub[1:].view(H0, W0)
    lv.copy_(torch.from_numpy(lab)), rv.copy_(torch.from_numpy(r)), uv.copy_(torch.from_numpy(u8))
    assert lv.data_ptr() % 16 == 4 and uv.data_ptr() % 4 == 1 and lv.is_contiguous()
    _compare(iu.region_stats(lv, rv, max_regions=40, nodata=-9999.0), ref.region_stats_ref(lab, r, max_regions=40, nodata=-9999.0), "off 4")
    _compare(iu.region_stats(lv, uv, max_regions=40), ref.region_stats_ref(lab, u8, max_regions=40), "uint8 off 1")


# ---- reproducibility -----------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_table_bytes(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import zonal
    lab, r = patches(H0, W0, 25), dirty_normal(H0, W0, 26)
    l, rr = torch.from_numpy(lab).to(dev), torch.from_numpy(r).to(dev)
    kw = dict(max_regions=40, nodata=-9999.0, bins=32, range=(-2.0, 2.0))
    sc = zonal.ZonalScratch(dev, 40, 32, 1)
    iu.region_stats(l, rr, scratch=sc, **kw)
    raw1 = sc.host.numpy().copy()
    iu.region_stats(l, rr, scratch=sc, **kw)
    raw2 = sc.host.numpy().copy()
    iu.region_stats(l, torch.from_numpy(dirty_normal(H0, W0, 27)).to(dev), scratch=sc, **kw)         # another raster in between
    fresh = zonal.ZonalScratch(dev, 40, 32, 1)
    fresh.table.fill_(0xFF)                                                                           # nothing relies on a cleared table
    iu.region_stats(l, rr, scratch=fresh, **kw)
    iu.region_stats(l, rr, scratch=sc, **kw)
    assert raw1.tobytes() == raw2.tobytes() == fresh.host.numpy().tobytes() == sc.host.numpy().tobytes()
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        iu.region_stats(l, rr, scratch=fresh, **kw)
    side.synchronize()
    assert raw1.tobytes() == fresh.host.numpy().tobytes()


# ---- with the stages around it -------------------------------------------------------------------------------------------
def test_consistent_with_label_regions(dev):
    import insar_unet_ca_amd as iu
    from tests.test_regions_gpu import striped_random
    mask = striped_random(H0, W0, 0.6, seed=41)
    conf = np.random.default_rng(42).random((H0, W0)).astype(np.float32)
    m, c = torch.from_numpy(mask).to(dev), torch.from_numpy(conf).to(dev)
    reg = iu.label_regions(m, c, connectivity=8, min_area=2)
    st = iu.region_stats(reg["labels"], c, scale=float(1 << 30), count=reg["count"])
    assert reg["count"] > 10 and st["out_of_range"] == 0
    assert (st["n"] == reg["regions"]["area"]).all() and (st["n_invalid"] == 0).all() and (st["n_clipped"] == 0).all()
    np.testing.assert_allclose(st["mean"], reg["regions"]["mean_conf"], rtol=1e-12, atol=0)
    _compare(st, ref.region_stats_ref(reg["labels"].cpu().numpy(), conf, scale=float(1 << 30), count=reg["count"]), "conf")


def test_detect_with_measure(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.data import make_tile
    T, o, H, W = 64, 8, 160, 208
    torch.manual_seed(5)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).train()
    crit, opt = iu.CrossEntropyLoss(ignore_index=255), iu.Adam(net.parameters(), lr=1e-3)
    data = iu.SyntheticTiles(12, size=T, channels=1)
    for step in range(3):
        items = [data[4 * step + i] for i in range(4)]
        opt.zero_grad()
        crit(net(torch.stack([it[0] for it in items]).to(dev)), torch.stack([it[1] for it in items]).to(dev)).backward()
        opt.step()
    rows = [np.concatenate([make_tile(7000 + 10 * r + c, T, 1)[0][0] for c in range((W + T - 1) // T)], axis=1)
            for r in range((H + T - 1) // T)]
    scene_f = np.ascontiguousarray(np.concatenate(rows, axis=0)[:H, :W])
    scene = np.clip(np.rint((scene_f * 0.5 + 0.5) * 255), 0, 255).astype(np.uint8)
    aux = np.random.default_rng(43).normal(size=(H, W)).astype(np.float32)
    pred = iu.ScenePredictor(net, tile=T, overlap=o, batch=4, num_classes=2)
    kw = dict(connectivity=8, min_area=3, min_conf=float(pred.predict(scene)["conf"].median()))
    plain = pred.detect(scene, **kw)
    assert "stats" not in plain and not pred._cached(iu.ZonalScratch)
    hist_kw = dict(bins=8, range=(-2.0, 2.0), nodata=0.0)
    det = pred.detect(scene, measure={"scene": "input", "aux": aux, "aux_dev": (torch.from_numpy(aux).to(dev), hist_kw)}, **kw)
    assert set(det) == set(plain) | {"stats"} and det["count"] == plain["count"] > 1
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, det[k]), k
    for k, v in plain["regions"].items():
        assert v.tobytes() == det["regions"][k].tobytes(), k
    by_hand = {"scene": iu.region_stats(det["labels"], torch.from_numpy(scene).to(dev), count=det["count"]),
               "aux": iu.region_stats(det["labels"], torch.from_numpy(aux).to(dev), count=det["count"]),
               "aux_dev": iu.region_stats(det["labels"], torch.from_numpy(aux).to(dev), count=det["count"], **hist_kw)}
    assert set(det["stats"]) == set(by_hand)
    for name, want in by_hand.items():
        got = det["stats"][name]
        assert set(got) == set(want)
        for f, v in want.items():
            if isinstance(v, np.ndarray):
                assert v.shape[0] == det["count"] and (v.tobytes() == got[f].tobytes() if v.dtype != object else (v == got[f]).all()), (name, f)
            else:
                assert got[f] == v, (name, f)
    assert (det["stats"]["scene"]["n"] == det["regions"]["area"]).all()
    assert det["stats"]["scene"]["max_q"].max() <= 255 and det["stats"]["scene"]["scale"] == 1.0
    _compare(det["stats"]["aux"], ref.region_stats_ref(det["labels"].cpu().numpy(), aux, count=det["count"]), "detect aux")
    one = iu.detect_scene(net, scene, tile=T, overlap=o, batch=4, num_classes=2, measure={"aux": aux}, **kw)
    assert one["stats"]["aux"]["sum_q"].tobytes() == det["stats"]["aux"]["sum_q"].tobytes()
    gt = (scene > 128).astype(np.uint8)
    ev = pred.evaluate(scene, gt, measure={"aux": aux}, **kw)
    assert ev["stats"]["aux"]["sum_q"].tobytes() == det["stats"]["aux"]["sum_q"].tobytes() and "score" in ev
    assert "stats" not in pred.evaluate(scene, gt, **kw)
    assert len(pred._cached(iu.ZonalScratch)) == 2
    pred.release()
    assert not pred._cached(iu.ZonalScratch)
