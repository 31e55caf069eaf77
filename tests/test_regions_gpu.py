"""GPU: regions of a class map (insar_unet_ca_amd/regions.py on csrc/regions.hip) against the scipy oracle of
tests/regions_ref.py (pinned against a flood fill in tests/test_regions_host.py).

Every comparison with the oracle is exact: labels, cleaned mask, count, class, area, box and the integer sums; cy / cx to
1e-12 relative (the same int64 sums divided in float64 on both sides). The scene is 200 x 264 unless a case says otherwise:
a work-group tile is 32 x 64 pixels, so that is 7 x 5 tiles, ragged on both axes against every power of two."""
import numpy as np
import pytest
import torch

from tests.regions_ref import foreground, quantise_conf, regions_oracle

pytestmark = pytest.mark.gpu
H0, W0 = 200, 264
INT_FIELDS = ("id", "cls", "area", "y0", "x0", "y1", "x1")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _compare(out, ref, with_conf, what=""):
    labels, clean = out["labels"].cpu().numpy(), out["mask"].cpu().numpy()
    assert out["labels"].dtype == torch.int32 and out["mask"].dtype == torch.uint8
    assert out["count"] == ref["count"], f"{what}: {out['count']} regions, oracle {ref['count']}"
    assert (labels == ref["labels"]).all(), f"{what}: {(labels != ref['labels']).sum()} labels differ"
    assert (clean == ref["mask"]).all(), what
    r, o = out["regions"], ref["regions"]
    for f in INT_FIELDS:
        assert r[f].shape == (ref["count"],) and (r[f] == o[f]).all(), f"{what}: {f}"
    assert r["area"].dtype == np.int64 and r["cy"].dtype == np.float64
    np.testing.assert_allclose(r["cy"], o["cy"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["cx"], o["cx"], rtol=1e-12, atol=0)
    assert ("mean_conf" in r) == with_conf
    print(f"{what}: {out['count']} regions, largest {int(r['area'].max(initial=0))} pixels")


def _check(dev, mask, conf=None, what="", **kw):
    import insar_unet_ca_amd as iu
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(dev)
    c = None if conf is None else torch.from_numpy(np.ascontiguousarray(conf, dtype=np.float32)).to(dev)
    out = iu.label_regions(m, c, **kw)
    okw = {k: v for k, v in kw.items() if k != "max_regions"}
    ref = regions_oracle(mask, conf, **okw)
    _compare(out, ref, conf is not None, what)
    assert (m.cpu().numpy() == mask).all()                       # the input is not written
    return out, ref


# ---- shapes ---------------------------------------------------------------------------------------------------------------
def serpentine(H, W):
    """A one-pixel path through every tile: every second row is full, joined alternately at the right and the left end."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def spiral(H, W):
    """A one-pixel wall winding inwards from (0, 0), one empty pixel between its turns: step ahead while the cell after the
    next is free, else turn right."""
    m = np.zeros((H, W), dtype=np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1

    def free(py, px):
        return not (0 <= py < H and 0 <= px < W) or m[py, px] == 0

    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and m[ny, nx] == 0 and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = ny, nx
        m[y, x] = 1


def nested_u(H, W):
    """U k: arms in columns 2k and W - 1 - 2k from row 0 down, joined only by its bottom row H - 1 - 2k."""
    m = np.zeros((H, W), dtype=np.uint8)
    for k in range(0, min(H, W) // 4, 2):
        m[0:H - 2 * k, 2 * k] = 1
        m[0:H - 2 * k, W - 1 - 2 * k] = 1
        m[H - 1 - 2 * k, 2 * k:W - 2 * k] = 1
    return m


def corner_blobs(H, W):
    """Two pairs of 10 x 10 blobs that touch only diagonally, each exactly at a corner shared by four tiles: one pair along
    the main diagonal at (64, 128), one along the anti-diagonal at (128, 192)."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[54:64, 118:128] = 1
    m[64:74, 128:138] = 1
    m[118:128, 192:202] = 1
    m[128:138, 182:192] = 1
    return m


def striped_random(H, W, fill, seed):
    """Random foreground at `fill`, three classes in adjacent 37-pixel stripes: class borders cut the blobs."""
    rng = np.random.default_rng(seed)
    cls = (1 + (np.arange(W) // 37) % 3).astype(np.uint8)
    return (rng.random((H, W)) < fill).astype(np.uint8) * cls[None, :]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", ["serpentine", "spiral", "nested_u"])
def test_long_chains(dev, shape, connectivity):
    m = {"serpentine": serpentine, "spiral": spiral, "nested_u": nested_u}[shape](H0, W0)
    out, ref = _check(dev, m, what=f"{shape}/{connectivity}", connectivity=connectivity)
    if shape == "serpentine":
        assert out["count"] == 1 and out["regions"]["area"][0] == int(m.sum())
    if shape == "nested_u":
        assert out["count"] == len(range(0, min(H0, W0) // 4, 2))


def test_diagonal_touch_at_a_four_tile_corner(dev):
    m = corner_blobs(H0, W0)
    out8, _ = _check(dev, m, what="corner/8", connectivity=8)
    out4, _ = _check(dev, m, what="corner/4", connectivity=4)
    assert out8["count"] == 2 and out4["count"] == 4
    assert out8["regions"]["area"].tolist() == [200, 200] and out4["regions"]["area"].tolist() == [100] * 4


def test_checkerboard(dev):
    yy, xx = np.indices((H0, W0))
    m = ((yy + xx) % 2 == 0).astype(np.uint8)
    out8, _ = _check(dev, m, what="checkerboard/8", connectivity=8, max_regions=65536)
    assert out8["count"] == 1 and out8["regions"]["area"][0] == 26400
    out4, _ = _check(dev, m, what="checkerboard/4", connectivity=4, max_regions=65536)
    assert out4["count"] == 26400 and (out4["regions"]["area"] == 1).all()
    out42, _ = _check(dev, m, what="checkerboard/4/min_area=2", connectivity=4, min_area=2, max_regions=65536)
    assert out42["count"] == 0 and int(out42["labels"].abs().sum()) == 0 and int(out42["mask"].sum()) == 0


@pytest.mark.parametrize("H, W, value", [(H0, W0, 0), (H0, W0, 1), (H0, W0, 7), (1, 300, 1), (300, 1, 1), (1, 1, 1), (1, 1, 0),
                                         (1, 300, None), (300, 1, None), (33, 65, None), (32, 64, 1)])
def test_uniform_and_degenerate_scenes(dev, H, W, value):
    if value is None:
        m = striped_random(H, W, 0.6, seed=H + W)
    else:
        m = np.full((H, W), value, dtype=np.uint8)
    for connectivity in (4, 8):
        out, _ = _check(dev, m, what=f"{H}x{W}/{value}/{connectivity}", connectivity=connectivity)
        if value is not None:
            assert out["count"] == (1 if value else 0)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("fill", [0.3, 0.5, 0.6, 0.8])
def test_random_masks_with_three_classes(dev, fill, connectivity):
    m = striped_random(H0, W0, fill, seed=int(fill * 10))
    out, _ = _check(dev, m, what=f"random {fill}/{connectivity}", connectivity=connectivity)
    assert set(np.unique(out["regions"]["cls"])) <= {1, 2, 3}


@pytest.mark.parametrize("H, W", [(201, 263), (199, 265)])
def test_widths_off_every_vector_boundary(dev, H, W):
    """W % 4 != 0 and H * W % 4 != 0: the scalar access paths of every kernel."""
    m = striped_random(H, W, 0.55, seed=W)
    conf = np.random.default_rng(W).random((H, W)).astype(np.float32)
    for connectivity in (4, 8):
        _check(dev, m, conf, what=f"{H}x{W}/{connectivity}", connectivity=connectivity, min_conf=0.25, min_area=2)


def test_a_scene_beyond_one_grid_and_one_scan_pass(dev):
    """2100 x 4100 = 8.6 M pixels: more than the 8192 x 1024 pixels one grid of the streaming kernels covers without looping,
    and 8409 numbering blocks, more than one pass of the 1024-thread scan. One region of millions of pixels."""
    rng = np.random.default_rng(3)
    m = (rng.random((2100, 4100)) < 0.55).astype(np.uint8)
    conf = (rng.integers(128, 1025, size=m.shape) / 1024.0).astype(np.float32)
    out, ref = _check(dev, m, conf, what="2100x4100", connectivity=8, min_area=4)
    assert out["regions"]["area"].max() > 4_000_000
    assert (out["regions"]["mean_conf"] == ref["regions"]["mean_conf"]).all()


# ---- filters and the region cap ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_area", [1, 5, 50])
def test_min_area_renumbers(dev, min_area):
    m = striped_random(H0, W0, 0.5, seed=11)
    out, ref = _check(dev, m, what=f"min_area={min_area}", connectivity=8, min_area=min_area)
    assert (out["regions"]["area"] >= min_area).all()
    assert (out["regions"]["id"] == np.arange(1, out["count"] + 1)).all()
    assert np.all(np.diff(ref["regions"]["root"]) > 0)           # ascending root order, with no gaps in the ids


@pytest.mark.parametrize("min_conf", [0.0, 0.4, 0.9])
def test_min_conf(dev, min_conf):
    m = striped_random(H0, W0, 0.7, seed=12)
    conf = np.random.default_rng(13).random((H0, W0)).astype(np.float32)
    out, _ = _check(dev, m, conf, what=f"min_conf={min_conf}", connectivity=8, min_conf=min_conf, min_area=3)
    clean = out["mask"].cpu().numpy()
    assert (clean[conf < np.float32(min_conf)] == 0).all()
    assert (foreground(m, conf, min_conf)[clean > 0] == clean[clean > 0]).all()


def test_region_cap_and_guard(dev):
    """max_regions = N passes; max_regions = N - 1 raises, and the bytes either side of the table stay untouched."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import regions
    from insar_unet_ca_amd._lib import InsarError
    mask = striped_random(H0, W0, 0.5, seed=21)
    ref = regions_oracle(mask, connectivity=4, min_area=2)
    N = ref["count"]
    assert N > 100
    m = torch.from_numpy(mask).to(dev)
    out = iu.label_regions(m, connectivity=4, min_area=2, max_regions=N)
    _compare(out, ref, False, "cap = N")
    with pytest.raises(InsarError, match=rf"{N} regions exceed max_regions={N - 1}"):
        iu.label_regions(m, connectivity=4, min_area=2, max_regions=N - 1)
    # the same through the phase calls, with the table inside a guard buffer
    cap = N - 1
    sb, tb = regions.scratch_bytes(H0, W0, cap)
    pad = 4096
    guard = torch.full((pad + tb + pad,), 0xA5, dtype=torch.uint8, device=dev)
    table = guard[pad:pad + tb]
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    labels = torch.empty(H0, W0, dtype=torch.int32, device=dev)
    clean = torch.empty(H0, W0, dtype=torch.uint8, device=dev)
    regions._launch(m, None, 4, 2, 0.0, cap, scratch, table, labels, clean)
    torch.cuda.synchronize()
    g = guard.cpu().numpy()
    assert (g[:pad] == 0xA5).all() and (g[pad + tb:] == 0xA5).all()
    rec = g[pad:pad + tb].view(regions.REGION_DTYPE)
    assert int(rec["area"][0]) == N                                 # the true count, beyond the cap
    assert (rec["area"][1:] == ref["regions"]["area"][:cap]).all() and (rec["root"][1:] == ref["regions"]["root"][:cap]).all()
    assert (labels.cpu().numpy() == ref["labels"]).all()            # labels are scene-sized: every id is written


# ---- confidence -----------------------------------------------------------------------------------------------------------
def test_integer_confidence_sums_are_exact(dev):
    """conf drawn as multiples of 2^-10 in [1/8, 1]: the int64 sums of llrint(conf * 2^30) equal the oracle's."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import regions
    mask = striped_random(H0, W0, 0.6, seed=31)
    conf = (np.random.default_rng(32).integers(128, 1025, size=(H0, W0)) / 1024.0).astype(np.float32)
    ref = regions_oracle(mask, conf, connectivity=8)
    sc = regions.RegionScratch(H0, W0, dev, 65536)
    out = iu.label_regions(torch.from_numpy(mask).to(dev), torch.from_numpy(conf).to(dev), connectivity=8, scratch=sc)
    _compare(out, ref, True, "conf 2^-10")
    rec = sc.host.numpy().view(regions.REGION_DTYPE)[1:1 + ref["count"]]
    assert (rec["sum_conf"] == ref["regions"]["sum_conf"]).all()
    assert (rec["sum_y"] == ref["regions"]["sum_y"]).all() and (rec["sum_x"] == ref["regions"]["sum_x"]).all()
    assert (out["regions"]["mean_conf"] == ref["regions"]["mean_conf"]).all()


def test_mean_conf_of_arbitrary_float32(dev):
    """Arbitrary float32 conf in [0, 1]: mean_conf within 1e-9 of the float64 mean (2^-31 per pixel from the rounding to
    2^-30, plus one division), and equal to the oracle's integer arithmetic exactly."""
    import insar_unet_ca_amd as iu
    mask = striped_random(H0, W0, 0.6, seed=41)
    conf = np.random.default_rng(42).random((H0, W0)).astype(np.float32)
    conf[0, :8] = [0.0, 1.0, 2.0 ** -31, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -30, 3 * 2.0 ** -31, 0.75]
    out, ref = _check(dev, mask, conf, what="conf float32", connectivity=8)
    assert (out["regions"]["mean_conf"] == ref["regions"]["mean_conf"]).all()
    labels = ref["labels"].ravel()
    exact = np.bincount(labels, weights=conf.astype(np.float64).ravel())[1:] / np.bincount(labels)[1:]
    err = np.abs(out["regions"]["mean_conf"] - exact).max()
    print(f"mean_conf: max error {err:.3e} against the float64 mean")
    assert err <= 1e-9


# ---- reproducibility and cleanliness -------------------------------------------------------------------------------------
def test_bitwise_repeatable_and_no_state_leaks(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import regions
    a = torch.from_numpy(striped_random(H0, W0, 0.6, seed=51)).to(dev)
    ca = torch.from_numpy(np.random.default_rng(52).random((H0, W0)).astype(np.float32)).to(dev)
    b = torch.from_numpy(serpentine(H0, W0) * np.uint8(2)).to(dev)
    kw = dict(connectivity=8, min_area=2, min_conf=0.2)
    sc = regions.RegionScratch(H0, W0, dev, 65536)
    first = iu.label_regions(a, ca, scratch=sc, **kw)
    raw1 = sc.host.numpy().copy()
    second = iu.label_regions(a, ca, scratch=sc, **kw)
    raw2 = sc.host.numpy().copy()
    assert torch.equal(first["labels"], second["labels"]) and torch.equal(first["mask"], second["mask"])
    assert first["labels"].data_ptr() != second["labels"].data_ptr()          # fresh tensors every call
    assert raw1.tobytes() == raw2.tobytes()
    # another scene through the same scratch, then the first again: equal to a call on fresh buffers
    iu.label_regions(b, None, scratch=sc, connectivity=4)
    again = iu.label_regions(a, ca, scratch=sc, **kw)
    raw3 = sc.host.numpy().copy()
    fresh_sc = regions.RegionScratch(H0, W0, dev, 65536)
    fresh_sc.scratch.fill_(0xFF), fresh_sc.table.fill_(0xFF)                  # nothing relies on cleared buffers
    fresh = iu.label_regions(a, ca, scratch=fresh_sc, **kw)
    for other, raw in ((again, raw3), (fresh, fresh_sc.host.numpy())):
        assert torch.equal(first["labels"], other["labels"]) and torch.equal(first["mask"], other["mask"])
        assert raw1.tobytes() == raw.tobytes()


def test_non_default_stream(dev):
    import insar_unet_ca_amd as iu
    mask = striped_random(H0, W0, 0.6, seed=61)
    conf = np.random.default_rng(62).random((H0, W0)).astype(np.float32)
    m, c = torch.from_numpy(mask).to(dev), torch.from_numpy(conf).to(dev)
    base = iu.label_regions(m, c, min_area=2, min_conf=0.1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        other = iu.label_regions(m, c, min_area=2, min_conf=0.1)
    side.synchronize()
    assert torch.equal(base["labels"], other["labels"]) and torch.equal(base["mask"], other["mask"])
    assert base["count"] == other["count"]
    for k, v in base["regions"].items():
        assert v.tobytes() == other["regions"][k].tobytes(), k


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_detect_is_predict_plus_label_regions(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.data import make_tile
    T, o, H, W = 64, 8, 160, 208
    torch.manual_seed(5)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).train()
    crit, opt = iu.CrossEntropyLoss(ignore_index=255), iu.Adam(net.parameters(), lr=1e-3)
    data = iu.SyntheticTiles(12, size=T, channels=1)
    for step in range(3):                                        # BatchNorm's running statistics leave their initial values
        items = [data[4 * step + i] for i in range(4)]
        opt.zero_grad()
        crit(net(torch.stack([it[0] for it in items]).to(dev)), torch.stack([it[1] for it in items]).to(dev)).backward()
        opt.step()
    rows = [np.concatenate([make_tile(7000 + 10 * r + c, T, 1)[0][0] for c in range((W + T - 1) // T)], axis=1)
            for r in range((H + T - 1) // T)]
    scene = np.ascontiguousarray(np.concatenate(rows, axis=0)[:H, :W])
    pred = iu.ScenePredictor(net, tile=T, overlap=o, batch=4, num_classes=2)
    before = pred.predict(scene, return_prob=True)
    # this net's winning probabilities lie in a narrow band above 1 / 2: threshold at their median, so that the confidence
    # filter cuts the class map into many regions
    kw = dict(connectivity=8, min_area=3, min_conf=float(before["conf"].median()))
    det = pred.detect(scene, return_prob=True, **kw)
    after = pred.predict(scene, return_prob=True)
    for k in ("mask", "conf", "prob"):
        assert torch.equal(before[k], det[k]) and torch.equal(before[k], after[k]), k
    ref = regions_oracle(det["mask"].cpu().numpy(), det["conf"].cpu().numpy(), **kw)
    got = {"labels": det["labels"], "mask": det["mask_clean"], "count": det["count"], "regions": det["regions"]}
    _compare(got, ref, True, "detect")
    assert det["count"] > 1
    assert (det["regions"]["mean_conf"] == ref["regions"]["mean_conf"]).all()
    one = iu.detect_scene(net, scene, return_prob=True, tile=T, overlap=o, batch=4, num_classes=2, **kw)
    for k in ("mask", "conf", "prob", "labels", "mask_clean"):
        assert torch.equal(det[k], one[k]), k
    assert one["count"] == det["count"] and all(one["regions"][k].tobytes() == v.tobytes() for k, v in det["regions"].items())
    assert len(pred._cached(iu.regions.RegionScratch)) == 1
    pred.release()
    assert not pred._cached(iu.regions.RegionScratch) and not pred._geom
