"""GPU: scenes with no-data (csrc/scene_valid.hip under insar_unet_ca_amd/infer.py) against the numpy restatement of
tests/scene_valid_ref.py. Everything is compared bit for bit: the census is a count, the gather a copy or two fp32 roundings
(uint8: the reference's transform, whose division hipcc rounds correctly), and at a valid pixel the masked predict adds the same
tiles in the same order as the plain predict of the scene whose invalid pixels carry the fill value, because with
min_valid = 1 every tile that covers a valid pixel is run (tests/test_scene_valid_host.py proves that on random masks).

Shapes: tile 32 (16 once), overlap 8, scenes up to 96 x 136: the flush-with-the-edge tile, W = 101 (rows that start off every
4-byte boundary; with H = 81 also an odd pixel count: the one-pixel-per-thread finalize) and W = 128 / 136 (quads) all occur."""
import math

import numpy as np
import pytest
import torch

from tests import scene_valid_ref as ref
from tests.helpers import record_calls

pytestmark = pytest.mark.gpu
TILE, OVERLAP = 32, 8
NAN, INF = np.float32("nan"), np.float32("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class _StubNet(torch.nn.Module):
    """Class 1 wherever the network input is positive: a pointwise function of x, hence the same logits for a tile whatever
    batch it comes in. One parameter, so that the predictor finds its device. Refuses a non-finite input and counts its tiles."""

    def __init__(self, check=True):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(4.0))
        self.seen, self.check = 0, check

    def forward(self, x):
        assert not self.check or bool(torch.isfinite(x).all()), "a non-finite value reached the net"
        self.seen += x.shape[0]
        return torch.cat([0.25 - x * x, self.gain * x], dim=1)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b) -> bool:
    a, b = _bits(a), _bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(a, b))


def _diagonal(H, W, half=14):
    """bool [H, W]: a band along the diagonal of the box; the two far corners hold nothing."""
    y, x = np.mgrid[0:H, 0:W]
    return np.abs(x - y * (W / H)) < half


def _scene(dtype, H, W, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    return rng.standard_normal((H, W)).astype(np.float32)


def _odd_table(H, W, tile):
    """A hand-made table: odd x0, the last legal origin, one tile twice, and two entries that are not inside the scene."""
    return np.array([[0, 1], [3, 5], [H - tile, W - tile], [H - tile - 1, 7], [3, 5], [H - tile + 1, 0], [-1, 3]], dtype=np.int32)


# scene dtype, (H, W), with a validity plane, nodata
INPUTS = [(np.uint8, (96, 136), False, 7), (np.uint8, (81, 101), True, None), (np.uint8, (64, 128), True, 0),
          (np.uint8, (81, 101), False, 255), (np.float32, (96, 136), False, None), (np.float32, (81, 101), True, -2.5),
          (np.float32, (64, 128), False, float("nan")), (np.float32, (81, 101), False, float("inf")),
          (np.float32, (64, 128), True, None)]


def _case(dtype, shape, plane, nodata, seed=0):
    """(scene, valid plane or None): a float32 scene carries NaN, +inf, -inf and the no-data value among its pixels."""
    H, W = shape
    rng = np.random.default_rng(seed + H + W)
    sc = _scene(dtype, H, W, seed)
    if dtype == np.float32:
        r = rng.random((H, W))
        sc[r < 0.10] = NAN
        sc[(r >= 0.10) & (r < 0.13)] = INF
        sc[(r >= 0.13) & (r < 0.16)] = -INF
        if nodata is not None and math.isfinite(nodata):
            sc[(r >= 0.16) & (r < 0.30)] = nodata
        sc[:40, :40] = NAN                                         # a whole tile of nothing
    elif nodata is not None:
        sc[rng.random((H, W)) < 0.2] = nodata
        sc[:40, :40] = nodata
    valid = None
    if plane:
        valid = (rng.integers(0, 4, size=(H, W)) * 85).astype(np.uint8)       # 0, 85, 170, 255: non-zero means observed
        valid[-36:, -36:] = 0
    return sc, valid


def _to(dev, a):
    return None if a is None else torch.from_numpy(a).to(dev)


# ---- census and gather -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, shape, plane, nodata", INPUTS)
def test_census_and_gather_against_the_restatement(dev, dtype, shape, plane, nodata):
    import insar_unet_ca_amd as iu
    H, W = shape
    sc, valid = _case(dtype, shape, plane, nodata)
    ok = ref.valid_pixels(sc, valid, nodata)
    assert 0 < ok.sum() < ok.size
    sc_d, valid_d = _to(dev, sc), _to(dev, valid)
    norm = (0.75, -3.0) if dtype == np.float32 and plane else None
    for tile, origins in ((TILE, iu.plan_tiles(H, W, TILE, OVERLAP)), (TILE, _odd_table(H, W, TILE)), (16, _odd_table(H, W, 16))):
        o_d = torch.from_numpy(origins).to(dev)
        counts = iu.tile_census(sc_d, o_d, tile, valid=valid_d, nodata=nodata)
        assert counts.dtype == torch.int32 and counts.shape == (len(origins),)
        want = ref.census(ok, origins, tile)
        assert np.array_equal(counts.cpu().numpy(), want), (counts.cpu().numpy(), want)
        got = iu.gather_tiles(sc_d, o_d, tile, valid=valid_d, nodata=nodata, fill=-0.375, norm=norm)
        assert bool(torch.isfinite(got).all())
        assert _same_bits(got, ref.gather_ref(sc, origins, tile, valid, nodata, fill=-0.375, norm=norm))
    assert want[-1] == 0 and want[-2] == 0 and want[1] == want[4]
    if (dtype, plane, nodata) == (np.uint8, False, 7):       # a census of zero and of a full tile both occur
        assert 0 in ref.census(ok, iu.plan_tiles(H, W, TILE, OVERLAP), TILE)


def test_norm_alone_selects_the_new_gather_and_nothing_else(dev, monkeypatch):
    import insar_unet_ca_amd as iu
    sc = _scene(np.float32, 64, 101, 3)
    origins = iu.plan_tiles(64, 101, TILE, OVERLAP)
    sc_d, o_d = _to(dev, sc), _to(dev, origins)
    got = iu.gather_tiles(sc_d, o_d, TILE, norm=(0.1, 1.7))
    assert _same_bits(got, ref.gather_ref(sc, origins, TILE, norm=(0.1, 1.7)))
    assert _same_bits(iu.gather_tiles(sc_d, o_d, TILE, fill=0.5), iu.gather_tiles(sc_d, o_d, TILE))        # all valid: no fill
    net = _StubNet().to(dev)
    pred = iu.ScenePredictor(net, tile=TILE, overlap=OVERLAP, batch=4)
    log = record_calls(monkeypatch)
    out = pred.predict(sc, norm=(0.1, 1.7))
    assert set(out) == {"mask", "conf"} and log.count("insar_scene_census") == 0 and log.count("insar_scene_finalize_valid") == 0
    assert log.count("insar_scene_gather_valid") == math.ceil(len(origins) / 4) and log.count("insar_scene_gather") == 0
    scaled = ((sc - np.float32(0.1)) * np.float32(1.7)).astype(np.float32)
    plain = pred.predict(scaled)
    assert _same_bits(out["mask"], plain["mask"]) and _same_bits(out["conf"], plain["conf"])


# ---- the masked predict against the plain predict of the filled scene --------------------------------------------------------
def _device_normalised(dev, byte):
    """What a uint8 pixel of this value is as network input: read off the plain gather."""
    import insar_unet_ca_amd as iu
    sc = torch.full((TILE, TILE), byte, dtype=torch.uint8, device=dev)
    return float(iu.gather_tiles(sc, torch.zeros(1, 2, dtype=torch.int32, device=dev), TILE)[0, 0, 0, 0])


FILL_BYTE = 191                # a uint8 scene's invalid pixels enter the net as this byte would: positive, class 1 to the stub
_PLAIN = {}


def _footprint_case(dev, dtype, shape, tta=1):
    """(scene, valid plane, nodata, fill, validity, the plain predict of the filled scene): computed once, shared, not written to."""
    import insar_unet_ca_amd as iu
    key = (dtype, shape, tta)
    if key not in _PLAIN:
        H, W = shape
        sc = _scene(dtype, H, W, 5)
        foot = _diagonal(H, W)
        if dtype == np.uint8:
            nodata, fill = 0, _device_normalised(dev, FILL_BYTE)
            valid = np.ones((H, W), dtype=np.uint8)
            valid[:, W // 2:] = foot[:, W // 2:]                   # right half: the plane; left half: the no-data value
            sc[:, :W // 2][~foot[:, :W // 2]] = 0
            filled = np.where(ref.valid_pixels(sc, valid, nodata), sc, np.uint8(FILL_BYTE)).astype(np.uint8)
        else:
            nodata, fill, valid = -2.5, 0.625, None
            sc[~foot] = NAN
            sc[5:9, 60:70] = INF
            sc[50:54, 60:66] = -INF
            sc[40:44, 50:60] = -2.5
            filled = np.where(ref.valid_pixels(sc, valid, nodata), sc, np.float32(fill)).astype(np.float32)
        ok = ref.valid_pixels(sc, valid, nodata)
        plain = iu.ScenePredictor(_StubNet().to(dev), tile=TILE, overlap=OVERLAP, batch=16 if tta == 1 else 1, tta=tta).predict(
            filled, return_prob=True)
        plain = {k: v.cpu().numpy() for k, v in plain.items()}
        assert plain["mask"][~ok].any()                            # the fill value is class 1 to the stub: the masking shows
        _PLAIN[key] = (sc, valid, nodata, fill, ok, plain)
    return _PLAIN[key]


def _check_masked(out, ok, plain, covered=None):
    want = ref.mask_outputs(plain, ok, np.ones_like(ok) if covered is None else covered)
    for k in ("mask", "conf", "prob", "valid"):
        assert _same_bits(out[k], want[k]), k
    keep = want["valid"].astype(bool)
    assert not out["mask"].cpu().numpy()[~keep].any() and not _bits(out["conf"])[~keep].any() and not _bits(out["prob"])[:, ~keep].any()


@pytest.mark.parametrize("batch", [1, 3, 16])
@pytest.mark.parametrize("dtype, shape", [(np.uint8, (96, 136)), (np.float32, (81, 101))])
def test_masked_predict_equals_the_plain_predict_of_the_filled_scene(dev, dtype, shape, batch):
    import insar_unet_ca_amd as iu
    sc, valid, nodata, fill, ok, plain = _footprint_case(dev, dtype, shape)
    net = _StubNet().to(dev)
    pred = iu.ScenePredictor(net, tile=TILE, overlap=OVERLAP, batch=batch)
    out = pred.predict(sc, return_prob=True, valid=valid, nodata=nodata, fill=fill)
    origins = iu.plan_tiles(*shape, TILE, OVERLAP)
    counts = ref.census(ok, origins, TILE)
    kept = iu.select_tiles(counts, 1)
    assert np.array_equal(out["tile_valid"], counts) and out["tile_valid"].dtype == np.int32
    assert out["tiles_total"] == len(origins) and out["tiles_run"] == len(kept) == net.seen < len(origins)
    assert type(out["tiles_run"]) is int and type(out["tiles_total"]) is int
    _check_masked(out, ok, plain)
    again = pred.predict(sc, return_prob=True, valid=_to(dev, valid), nodata=nodata, fill=fill)      # the cached buffers, a device plane
    for k in ("mask", "conf", "prob", "valid"):
        assert _same_bits(out[k], again[k]), k


def test_tta_masked_equals_plain_tta_of_the_filled_scene(dev):
    """batch = 1 on both sides: with tta > 1 a pixel's contributions are added batch by batch and, within a batch, op by op
    (infer.py: reproducible "for a fixed batch and tta"), so the order depends on which tiles share a batch, and skipping
    tiles changes that. One tile per batch takes the composition out: tile by tile, op by op, on both sides."""
    import insar_unet_ca_amd as iu
    sc, valid, nodata, fill, ok, plain = _footprint_case(dev, np.float32, (81, 101), tta=4)
    net = _StubNet().to(dev)
    out = iu.ScenePredictor(net, tile=TILE, overlap=OVERLAP, batch=1, tta=4).predict(sc, return_prob=True, nodata=nodata, fill=fill)
    assert net.seen == 4 * out["tiles_run"] and out["tiles_run"] < out["tiles_total"]
    _check_masked(out, ok, plain)


def test_one_valid_pixel_in_the_corner_of_four_tiles(dev):
    import insar_unet_ca_amd as iu
    H, W = 96, 136
    sc = _scene(np.uint8, H, W, 6)
    valid = np.zeros((H, W), dtype=np.uint8)
    valid[27, 28] = 1                                   # rows 24..31 and columns 24..31 lie under two tiles each
    net = _StubNet().to(dev)
    out = iu.ScenePredictor(net, tile=TILE, overlap=OVERLAP, batch=16).predict(sc, valid=valid, return_prob=True)
    assert out["tiles_run"] == 4 == net.seen and out["tile_valid"].sum() == 4 and set(out["tile_valid"]) == {0, 1}
    v = out["valid"].cpu().numpy()
    assert v.sum() == 1 and v[27, 28] == 1
    full = iu.ScenePredictor(_StubNet().to(dev), tile=TILE, overlap=OVERLAP, batch=16).predict(sc, return_prob=True)
    for k in ("mask", "conf"):
        got = out[k].cpu().numpy()
        assert _same_bits(got[27, 28], full[k].cpu().numpy()[27, 28]) and np.count_nonzero(got) <= 1
    assert _same_bits(out["prob"][:, 27, 28], full["prob"][:, 27, 28]) and out["conf"][27, 28].item() > 0


def test_all_invalid_scene_runs_no_forward(dev):
    import insar_unet_ca_amd as iu
    sc = np.full((64, 101), NAN, dtype=np.float32)
    net = _StubNet().to(dev)
    pred = iu.ScenePredictor(net, tile=TILE, overlap=OVERLAP, batch=4)
    for kw in (dict(nodata=float("nan")), dict(valid=np.ones((64, 101), dtype=np.uint8))):
        out = pred.predict(sc, return_prob=True, **kw)
        assert net.seen == 0 and out["tiles_run"] == 0 and out["tiles_total"] == 12 and not out["tile_valid"].any()
        for k in ("mask", "conf", "prob", "valid"):
            assert not _bits(out[k]).any(), k
    assert out["mask"].dtype == torch.uint8 and out["valid"].dtype == torch.uint8 and out["valid"].shape == (64, 101)


@pytest.mark.parametrize("shape", [(96, 136), (81, 101)])
def test_all_valid_scene_through_the_masked_path_is_the_plain_predict(dev, shape):
    import insar_unet_ca_amd as iu
    sc = np.minimum(_scene(np.uint8, *shape, 7), 254).astype(np.uint8)
    pred = iu.ScenePredictor(_StubNet().to(dev), tile=TILE, overlap=OVERLAP, batch=5)
    plain = pred.predict(sc, return_prob=True)
    out = pred.predict(sc, return_prob=True, nodata=255)
    assert out["tiles_run"] == out["tiles_total"] == len(iu.plan_tiles(*shape, TILE, OVERLAP))
    assert (out["tile_valid"] == TILE * TILE).all() and bool((out["valid"] == 1).all())
    for k in ("mask", "conf", "prob"):
        assert _same_bits(out[k], plain[k]), k
    assert "prob" not in pred.predict(sc, nodata=255)


def test_min_valid_above_one_leaves_valid_pixels_uncovered(dev):
    import insar_unet_ca_amd as iu
    H, W, min_valid = 96, 136, 10
    sc = _scene(np.float32, H, W, 8)
    valid = np.zeros((H, W), dtype=np.uint8)
    valid[:50, :60] = 1
    valid[90:93, 130:133] = 1                            # nine pixels in the far corner: its tile is one short
    sc[10:20, 10:20] = NAN
    ok = ref.valid_pixels(sc, valid, None)
    origins = iu.plan_tiles(H, W, TILE, OVERLAP)
    counts = ref.census(ok, origins, TILE)
    kept = iu.select_tiles(counts, min_valid)
    cov = ref.covered(origins[kept], TILE, H, W)
    assert ((counts > 0) & (counts < min_valid)).any() and (ok & ~cov).any() and (ok & cov).any()        # not vacuous
    net = _StubNet().to(dev)
    out = iu.ScenePredictor(net, tile=TILE, overlap=OVERLAP, batch=3).predict(sc, return_prob=True, valid=valid, min_valid=min_valid,
                                                                               fill=0.625)
    assert out["tiles_run"] == len(kept) == net.seen and np.array_equal(out["tile_valid"], counts)
    x = torch.from_numpy(ref.gather_ref(sc, origins[kept], TILE, valid, None, fill=0.625)).to(dev)
    with torch.no_grad():
        logits = _StubNet().to(dev)(x)
    st = iu.stitch_logits(logits, origins[kept], H, W, TILE, OVERLAP)
    _check_masked(out, ok, {k: v.cpu().numpy() for k, v in st.items()}, cov)
    assert out["valid"].cpu().numpy()[90:93, 130:133].sum() == 0 and st["mask"].cpu().numpy()[~ok & cov].any()


def test_real_unet_on_a_scene_with_nan_nodata(dev):
    """The defect on the plain path, as it shows on the device. This package's U-Net does not hand a NaN on: its BatchNorm+ReLU
    kernels form fmaxf(z, 0), which is 0 for a NaN, so the first unit turns the NaN band into finite values that mean nothing
    (measured on an MI355X: 0 of the 4608 pixels of this scene with a non-finite conf, 2064 of them no-data, and the conf of
    valid pixels next to the no-data changed). A net whose operations keep a NaN (torch's own do) sends it through the blend's
    fma into every pixel its tiles overlap: non-finite conf. Both are pinned here; the masked path shows neither."""
    import insar_unet_ca_amd as iu
    from oracle import closed_form as cf
    H, W = 64, 72
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True)
    net.load_state_dict(cf.fill_state_dict_random(net.state_dict(), seed=7))
    net = net.to(dev).eval()
    sc = (0.5 * _scene(np.float32, H, W, 9)).astype(np.float32)
    sc[:, 40:] = NAN                                     # the tiles at x0 = 40 hold nothing
    sc[30:34, 10:14] = NAN
    ok = ref.valid_pixels(sc, None, float("nan"))
    assert 0 < ok.sum() < ok.size
    pred = iu.ScenePredictor(net, tile=TILE, overlap=OVERLAP, batch=1)
    out = pred.predict(sc, return_prob=True, nodata=float("nan"), fill=0.0)
    for k in ("conf", "prob"):
        assert bool(torch.isfinite(out[k]).all()), k
    assert 0 < out["tiles_run"] < out["tiles_total"]
    filled = np.where(ok, sc, np.float32(0.0)).astype(np.float32)
    plain = {k: v.cpu().numpy() for k, v in pred.predict(filled, return_prob=True).items()}
    _check_masked(out, ok, plain)
    broken = pred.predict(sc)["conf"]
    n_bad = int((~torch.isfinite(broken)).sum())
    n_wrong = int(((_bits(broken) != _bits(plain["conf"])) & ok).sum())
    print(f"plain predict of the NaN scene: {n_bad} of {H * W} pixels with a non-finite conf, {int((~ok).sum())} are no-data, "
          f"{n_wrong} valid pixels with another conf than the filled scene gives")
    assert n_wrong > 0
    leaky = iu.ScenePredictor(_StubNet(check=False).to(dev), tile=TILE, overlap=OVERLAP, batch=1)
    n_bad = int((~torch.isfinite(leaky.predict(sc)["conf"])).sum())
    print(f"plain predict of the NaN scene with a net that keeps a NaN: {n_bad} pixels with a non-finite conf")
    assert n_bad >= int((~ok).sum())
    assert bool(torch.isfinite(leaky.predict(sc, nodata=float("nan"))["conf"]).all())


# ---- launches ------------------------------------------------------------------------------------------------------------
NEW = ("insar_scene_census", "insar_scene_gather_valid", "insar_scene_finalize_valid")


def test_defaults_launch_what_they_did_and_the_masked_path_its_own(dev, monkeypatch):
    import insar_unet_ca_amd as iu
    sc, valid, nodata, fill, ok, _ = _footprint_case(dev, np.uint8, (96, 136))
    pred = iu.ScenePredictor(_StubNet().to(dev), tile=TILE, overlap=OVERLAP, batch=5)
    origins = iu.plan_tiles(96, 136, TILE, OVERLAP)
    log = record_calls(monkeypatch)
    pred.predict(sc)
    n_batches = math.ceil(len(origins) / 5)
    assert all(log.count(n) == 0 for n in NEW)
    assert log.names() == ["insar_scene_gather", "insar_scene_blend"] * n_batches + ["insar_scene_finalize"]
    del log[:]
    iu.gather_tiles(_to(dev, sc), _to(dev, origins), TILE)
    assert log.names() == ["insar_scene_gather"]
    del log[:]
    out = pred.predict(sc, valid=valid, nodata=nodata, fill=fill)
    n_batches = math.ceil(out["tiles_run"] / 5)
    assert 0 < out["tiles_run"] < len(origins)
    assert log.names() == ["insar_scene_census"] + ["insar_scene_gather_valid", "insar_scene_blend"] * n_batches + ["insar_scene_finalize_valid"]


# ---- plumbing ------------------------------------------------------------------------------------------------------------
def _blobs(H=96, W=136):
    """A dark uint8 scene (class 0 to the stub) with two bright squares; the right part of the box is no-data (0)."""
    sc = np.full((H, W), 60, dtype=np.uint8)
    sc[20:32, 20:34] = 220                               # A: in the valid area
    sc[:, 90:] = 0                                       # no-data; B would lie at [50:62, 100:116]
    return sc


def test_detect_finds_no_region_in_the_invalid_area(dev):
    import insar_unet_ca_amd as iu
    sc = _blobs()
    fill = _device_normalised(dev, FILL_BYTE)            # class 1 to the stub: unmasked, the no-data area would be one big region
    det = iu.detect_scene(_StubNet().to(dev), sc, tile=TILE, overlap=OVERLAP, batch=4, nodata=0, fill=fill)
    assert det["count"] == 1 and not det["labels"].cpu().numpy()[:, 90:].any() and not det["mask"].cpu().numpy()[:, 90:].any()
    assert det["labels"].cpu().numpy()[20:32, 20:34].all() and not det["valid"].cpu().numpy()[:, 90:].any()
    assert det["tiles_run"] < det["tiles_total"]


def test_evaluate_voids_the_ground_truth_in_the_invalid_area(dev):
    import insar_unet_ca_amd as iu
    sc = _blobs()
    gt = np.zeros(sc.shape, dtype=np.uint8)
    gt[20:32, 20:34] = 1
    gt[50:62, 100:116] = 1                               # B: wholly inside the no-data area
    pred = iu.ScenePredictor(_StubNet().to(dev), tile=TILE, overlap=OVERLAP, batch=4)
    ev = pred.evaluate(sc, gt, nodata=0, fill=_device_normalised(dev, FILL_BYTE))
    assert ev["gt_count"] == 1 and ev["count"] == 1
    overall = ev["score"]["overall"]
    assert (overall["tp"], overall["fp"], overall["fn"]) == (1, 0, 0)
    assert ev["score"]["gt_match"].tolist() == [1] and not ev["gt_labels"].cpu().numpy()[:, 90:].any()
    full = pred.evaluate(np.where(sc == 0, np.uint8(60), sc), gt)                # the same scene observed everywhere: B is a miss
    assert full["gt_count"] == 2 and full["score"]["overall"]["fn"] == 1


def test_detect_stack_takes_a_dates_nodata_as_not_observed(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.stack import DetectionStack, follow_sites
    H, W = 64, 101
    base = np.full((H, W), 60, dtype=np.uint8)
    base[10:20, 10:22] = 220                             # site 1
    base[40:50, 70:82] = 220                             # site 2
    mid = base.copy()
    mid[5:30, 5:30] = 0                                  # the middle date does not observe site 1
    scenes = [base, mid, base]
    extra = np.ones((H, W), dtype=np.uint8)
    extra[40:50, 70:76] = 0                              # and the caller's own map hides half of site 2 on that date
    valids = [None, extra, None]
    pred = iu.ScenePredictor(_StubNet().to(dev), tile=TILE, overlap=OVERLAP, batch=4)
    res = pred.detect_stack(scenes, valids=valids, nodata=0, min_run=2)
    st = DetectionStack(H, W, dev, 1)
    for sc, v in zip(scenes, valids):
        out = pred.predict(sc, nodata=0)
        ok = ref.valid_pixels(sc, v, 0)
        assert np.array_equal(out["valid"].cpu().numpy(), ref.valid_pixels(sc, None, 0).astype(np.uint8))
        st.push(out["mask"], conf=out["conf"], valid=torch.from_numpy(ok.astype(np.uint8)).to(dev))
    want = follow_sites(st, min_run=2)
    assert res["count"] == want["count"] == 2
    for k, v in want["summary"].items():
        assert _same_bits(res["summary"][k], v), k
    n_valid, run = res["summary"]["n_valid"].cpu().numpy(), res["summary"]["longest_run"].cpu().numpy()
    assert (n_valid[10:20, 10:22] == 2).all() and (run[10:20, 10:22] == 2).all()          # unobserved: the run is not broken
    assert (run[40:50, 70:76] == 2).all() and (run[40:50, 76:82] == 3).all()
    assert (n_valid[40:50, 70:76] == 2).all() and (n_valid[40:50, 76:82] == 3).all()
    broken = pred.detect_stack(scenes, min_run=2)                                          # unmasked: observed, no hit
    assert (broken["summary"]["longest_run"].cpu().numpy()[10:20, 10:22] == 1).all() and broken["count"] == 1
