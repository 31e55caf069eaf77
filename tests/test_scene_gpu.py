"""GPU: whole-scene inference (insar_unet_ca_amd/infer.py on csrc/scene.hip). The stitch is held against the float64
restatement in tests/test_scene_host.py (pinned there against a brute-force loop) on synthetic logits, and bit for bit
against itself across batch sizes; the predictor is held against the eval-mode forward of the net it wraps.

Tolerances (all absolute, values in [0, 1]): prob / conf 3e-6 = twice the worst case of some twenty-five fp32 roundings
(a softmax of about five, at most nine multiply-adds, one divide; 25 * 6e-8 = 1.5e-6); mask compared where the yardstick's
top two probabilities differ by more than 1e-5 (over three times the prob tolerance on each side), and the pixels that this
margin leaves out may be at most 0.1 % of the scene."""
import numpy as np
import pytest
import torch

from tests.test_scene_host import stitch_oracle

pytestmark = pytest.mark.gpu
T = 256
PROB_TOL = 3e-6
MARGIN = 1e-5
MAX_EXCLUDED = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _u8_scene(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


def _host_normalise(v):
    x = v.astype(np.float32) / np.float32(255.0)
    return (x - np.float32(0.5)) / np.float32(0.5)


def _bitwise(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a, b))


def _check_mask(mask, ref_prob, what):
    """mask [H, W] against argmax of ref_prob [K, H, W] (numpy) wherever the top two differ by more than MARGIN."""
    srt = np.sort(ref_prob, axis=0)
    clear = (srt[-1] - srt[-2]) > MARGIN
    excluded = 1.0 - clear.mean()
    wrong = int(((mask != ref_prob.argmax(axis=0)) & clear).sum())
    print(f"{what}: {excluded:.2e} of the pixels inside the {MARGIN:g} margin, {wrong} clear pixels differ")
    assert excluded <= MAX_EXCLUDED
    assert wrong == 0


# ---- gather --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", [(600, 700), (600, 701)])        # 701: rows that start off every 4-byte boundary
def test_gather_uint8_and_float32(dev, H, W):
    import insar_unet_ca_amd as iu
    origins = iu.plan_tiles(H, W, T, 32)
    o_dev = torch.from_numpy(origins).to(dev)
    sc = _u8_scene(H, W, 3)
    got = iu.gather_tiles(torch.from_numpy(sc).to(dev), o_dev, T)
    assert got.shape == (len(origins), 1, T, T) and got.dtype == torch.float32
    want = np.stack([_host_normalise(sc[y:y + T, x:x + T]) for y, x in origins])[:, None]
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"gather uint8 {H}x{W}: max abs err {err:.2e}")
    assert err <= 1e-6
    assert got.min().item() == -1.0 and got.max().item() == 1.0
    # the float32 path copies
    scf = np.random.default_rng(4).standard_normal((H, W)).astype(np.float32)
    gotf = iu.gather_tiles(torch.from_numpy(scf).to(dev), o_dev, T)
    wantf = np.stack([scf[y:y + T, x:x + T] for y, x in origins])[:, None]
    assert np.array_equal(gotf.cpu().numpy().view(np.uint32), wantf.view(np.uint32))


# ---- stitch against the float64 oracle ----------------------------------------------------------------------------
STITCH_CASES = [(600, 700, 2, 32), (714, 600, 2, 32), (768, 768, 5, 128), (600, 700, 5, 0), (714, 600, 2, 128)]


def _synthetic_logits(seed, N, K, tile=T):
    return np.random.default_rng(seed).standard_normal((N, K, tile, tile)).astype(np.float32)


def _against_oracle(dev, H, W, K, o, seed, tile=T, chunk=None):
    import insar_unet_ca_amd as iu
    origins = iu.plan_tiles(H, W, tile, o)
    lg = _synthetic_logits(seed, len(origins), K, tile)
    out = iu.stitch_logits(torch.from_numpy(lg).to(dev), origins, H, W, tile, o, chunk=chunk)
    assert out["prob"].shape == (K, H, W) and out["prob"].dtype == torch.float32
    assert out["conf"].shape == (H, W) and out["conf"].dtype == torch.float32
    assert out["mask"].shape == (H, W) and out["mask"].dtype == torch.uint8
    prob, conf, mask = (out[k].cpu().numpy() for k in ("prob", "conf", "mask"))
    ref, wsum = stitch_oracle(lg, origins, H, W, tile, o)
    assert (wsum > 0).all()
    e_prob = np.abs(prob - ref).max()
    e_conf = np.abs(conf - ref.max(axis=0)).max()
    e_sum = np.abs(prob.astype(np.float64).sum(axis=0) - 1.0).max()
    print(f"stitch {H}x{W} K={K} o={o}: prob err {e_prob:.2e}, conf err {e_conf:.2e}, |sum - 1| {e_sum:.2e}")
    assert e_prob <= PROB_TOL and e_conf <= PROB_TOL
    assert e_sum <= 1e-6
    _check_mask(mask, ref, f"stitch {H}x{W} K={K} o={o}")
    # conf is the probability of the class the mask names
    assert np.array_equal(conf, np.take_along_axis(prob, mask[None].astype(np.int64), axis=0)[0])


@pytest.mark.parametrize("seed, case", list(enumerate(STITCH_CASES)))
def test_stitch_against_float64_oracle(dev, seed, case):
    H, W, K, o = case
    _against_oracle(dev, H, W, K, o, seed)


@pytest.mark.parametrize("H, W, K, o, tile, chunk", [(300, 333, 3, 20, 64, 7), (131, 205, 8, 32, 64, 4), (97, 130, 7, 5, 32, None)])
def test_stitch_unaligned_widths_and_more_classes(dev, H, W, K, o, tile, chunk):
    """W % 4 != 0 takes the one-pixel-per-thread kernels, overlaps that are not multiples of 4 the element-wise logit
    loads; K up to the cap of 8. Same oracle, same tolerances."""
    _against_oracle(dev, H, W, K, o, seed=11, tile=tile, chunk=chunk)


def test_stitch_without_prob(dev):
    import insar_unet_ca_amd as iu
    H, W, K, o = 600, 700, 2, 32
    origins = iu.plan_tiles(H, W, T, o)
    lg = torch.from_numpy(_synthetic_logits(0, len(origins), K)).to(dev)
    a = iu.stitch_logits(lg, origins, H, W, T, o, return_prob=True)
    b = iu.stitch_logits(lg, origins, H, W, T, o, return_prob=False)
    assert "prob" not in b and _bitwise(a["mask"], b["mask"]) and _bitwise(a["conf"], b["conf"])


# ---- determinism ---------------------------------------------------------------------------------------------------------
def test_stitch_is_bitwise_independent_of_the_chunk(dev):
    import insar_unet_ca_amd as iu
    H, W, K, o = 714, 600, 2, 128                   # has the nine-deep pixels
    origins = iu.plan_tiles(H, W, T, o)
    N = len(origins)
    lg = torch.from_numpy(_synthetic_logits(4, N, K)).to(dev)
    base = iu.stitch_logits(lg, origins, H, W, T, o, chunk=N)
    for chunk in (1, 5, 16, N, N):                   # N twice more: two repeats of one configuration
        out = iu.stitch_logits(lg, origins, H, W, T, o, chunk=chunk)
        for k in ("prob", "conf", "mask"):
            assert _bitwise(base[k], out[k]), f"chunk={chunk}: {k} differs"
    rep = iu.stitch_logits(lg, origins, H, W, T, o, chunk=5)
    again = iu.stitch_logits(lg, origins, H, W, T, o, chunk=5)
    for k in ("prob", "conf", "mask"):
        assert _bitwise(rep[k], again[k])


# ---- the net in the loop ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained_unet(dev):
    """UNet(use_se=True) fp32, seeded weights, three training steps on SyntheticTiles: BatchNorm's running statistics
    are no longer the initial ones."""
    import insar_unet_ca_amd as iu
    torch.manual_seed(5)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).train()
    crit = iu.CrossEntropyLoss(ignore_index=255)
    opt = iu.Adam(net.parameters(), lr=1e-3)
    data = iu.SyntheticTiles(12, size=T, channels=1)
    for step in range(3):
        items = [data[4 * step + i] for i in range(4)]
        x = torch.stack([it[0] for it in items]).to(dev)
        y = torch.stack([it[1] for it in items]).to(dev)
        opt.zero_grad()
        crit(net(x), y).backward()
        opt.step()
    torch.cuda.synchronize()
    assert float(net.inc.double_conv[1].running_mean.abs().max()) > 0
    return net


def _synthetic_scene(H, W):
    """float32 scene in [-1, 1] made of the package's synthetic interferogram tiles (what the net was trained on)."""
    from insar_unet_ca_amd.data import make_tile
    rows = []
    for r in range((H + T - 1) // T):
        rows.append(np.concatenate([make_tile(5000 + 10 * r + c, T, 1)[0][0] for c in range((W + T - 1) // T)], axis=1))
    return np.ascontiguousarray(np.concatenate(rows, axis=0)[:H, :W])


def test_predict_without_overlap_is_the_nets_softmax(dev, trained_unet):
    """prob of predict(tile=256, overlap=0, batch=4) on a 512 x 768 scene = softmax of the same eval-mode net on the same
    batches, tile by tile. Observed on an MI355X: prob and conf equal the yardstick bit for bit (w = 1 and wsum = 1 are
    exact); this net's probabilities lie in [0.477, 0.523] and no pixel falls inside the 1e-5 margin (share 0; cap 0.1 %)."""
    import insar_unet_ca_amd as iu
    H, W = 512, 768
    scene = _synthetic_scene(H, W)
    pred = iu.ScenePredictor(trained_unet, tile=T, overlap=0, batch=4, num_classes=2)
    out = pred.predict(scene, return_prob=True)
    origins = iu.plan_tiles(H, W, T, 0)
    assert len(origins) == 6
    ref = np.zeros((2, H, W), dtype=np.float32)
    trained_unet.eval()
    with torch.no_grad():
        for i in range(0, 6, 4):
            o = origins[i:i + 4]
            x = torch.from_numpy(np.stack([scene[y:y + T, x0:x0 + T] for y, x0 in o])[:, None]).to(dev)
            p = torch.softmax(trained_unet(x), 1).cpu().numpy()
            for j, (y, x0) in enumerate(o):
                ref[:, y:y + T, x0:x0 + T] = p[j]
    trained_unet.train()
    prob, conf, mask = (out[k].cpu().numpy() for k in ("prob", "conf", "mask"))
    e_prob, e_conf = np.abs(prob - ref).max(), np.abs(conf - ref.max(axis=0)).max()
    print(f"predict o=0: prob err {e_prob:.2e}, conf err {e_conf:.2e}, prob range [{ref.min():.3f}, {ref.max():.3f}]")
    assert e_prob <= PROB_TOL and e_conf <= PROB_TOL
    _check_mask(mask, ref, "predict o=0")


def test_predict_with_overlap_is_stitch_of_the_nets_logits(dev, trained_unet):
    import insar_unet_ca_amd as iu
    H, W, o, batch = 600, 700, 32, 4
    scene = _u8_scene(H, W, 9)
    out = iu.ScenePredictor(trained_unet, tile=T, overlap=o, batch=batch, num_classes=2).predict(scene, return_prob=True)
    origins = iu.plan_tiles(H, W, T, o)
    o_dev = torch.from_numpy(origins).to(dev)
    sc = torch.from_numpy(scene).to(dev)
    trained_unet.eval()
    with torch.no_grad():
        logits = torch.cat([trained_unet(iu.gather_tiles(sc, o_dev[i:i + batch], T)) for i in range(0, len(origins), batch)])
    trained_unet.train()
    ref = iu.stitch_logits(logits, origins, H, W, T, o, chunk=batch)
    for k in ("prob", "conf", "mask"):
        assert _bitwise(out[k], ref[k]), k
    other = iu.stitch_logits(logits, origins, H, W, T, o, chunk=None)
    for k in ("prob", "conf", "mask"):
        assert _bitwise(out[k], other[k]), k


def test_accumulators_are_cleared_between_calls(dev, trained_unet):
    import insar_unet_ca_amd as iu
    pred = iu.ScenePredictor(trained_unet, tile=T, overlap=32, batch=4, num_classes=2)
    scene = _u8_scene(600, 700, 21)
    a = pred.predict(scene, return_prob=True)
    b = pred.predict(scene, return_prob=True)
    pred.predict(_u8_scene(512, 768, 22), return_prob=True)          # another geometry in between
    c = pred.predict(torch.from_numpy(scene).to(dev), return_prob=True)      # and a device scene this time
    for k in ("prob", "conf", "mask"):
        assert a[k].data_ptr() != b[k].data_ptr()
        assert _bitwise(a[k], b[k]) and _bitwise(a[k], c[k]), k
    assert trained_unet.training                                       # restored
    one_shot = iu.predict_scene(trained_unet, scene, return_prob=True, tile=T, overlap=32, batch=4)
    assert _bitwise(a["prob"], one_shot["prob"])


def _make_net(name):
    import insar_unet_ca_amd as iu
    bf16 = torch.bfloat16
    torch.manual_seed(31)
    if name == "UNet":
        return iu.UNet(in_channels=1, num_classes=2, use_se=True, compute_dtype=bf16)
    if name == "UNetSpatialAttention":
        return iu.UNetSpatialAttention(in_channels=1, num_classes=2, compute_dtype=bf16)
    return getattr(iu, name)(num_classes=2, backbone="resnet50", pretrained=False, compute_dtype=bf16)


@pytest.mark.parametrize("name", ["UNet", "UNetSpatialAttention", "DeepLabV3_SingleChannel_Attn", "FCN_SingleChannel",
                                  "FCN_SingleChannel_SE"])
def test_every_exported_net_runs(dev, name):
    import insar_unet_ca_amd as iu
    net = _make_net(name).to(dev)
    H, W, K = 256, 512, 2
    scene = _u8_scene(H, W, 40)
    pred = iu.ScenePredictor(net, tile=T, overlap=32, batch=3, num_classes=K)
    for mode in (True, False):
        net.train(mode)
        out = pred.predict(scene, return_prob=True)
        assert net.training is mode
        assert out["mask"].shape == (H, W) and out["mask"].dtype == torch.uint8 and out["mask"].is_cuda
        assert out["conf"].shape == (H, W) and out["conf"].dtype == torch.float32
        assert out["prob"].shape == (K, H, W) and out["prob"].dtype == torch.float32
        assert bool(torch.isfinite(out["prob"]).all())
        assert float(out["conf"].min()) >= 1.0 / K - 1e-6 and float(out["conf"].max()) <= 1.0 + 1e-6
        assert float((out["prob"].sum(0) - 1.0).abs().max()) <= 1e-6
        assert int(out["mask"].max()) < K
        assert all(p.grad is None for p in net.parameters())
    assert "prob" not in pred.predict(scene)


# ---- refusals (host-side checks; nothing is launched) ------------------------------------------------------------
def test_refusals(dev, trained_unet):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import InsarError
    pred = iu.ScenePredictor(trained_unet, tile=T, overlap=32, batch=4)
    with pytest.raises(InsarError, match="smaller than the tile"):
        pred.predict(np.zeros((200, 700), dtype=np.uint8))
    with pytest.raises(InsarError, match="overlap"):
        iu.ScenePredictor(trained_unet, tile=T, overlap=T // 2 + 1)
    with pytest.raises(InsarError, match="2-D"):
        pred.predict(np.zeros((1, 600, 700), dtype=np.uint8))
    with pytest.raises(InsarError, match="dtype"):
        pred.predict(np.zeros((600, 700), dtype=np.float64))
    with pytest.raises(InsarError, match="dtype"):
        pred.predict(torch.zeros(600, 700, dtype=torch.float64, device=dev))
    lg = torch.zeros(9, 2, T, T, device=dev)
    origins = iu.plan_tiles(600, 700, T, 32)
    with pytest.raises(InsarError, match="leaves the"):
        iu.stitch_logits(lg, origins + 500, 600, 700, T, 32)
    with pytest.raises(InsarError, match="origins"):
        iu.stitch_logits(lg, origins[:5], 600, 700, T, 32)
    with pytest.raises(InsarError, match="num_classes"):
        iu.stitch_logits(torch.zeros(9, 9, T, T, device=dev), origins, 600, 700, T, 32)
    with pytest.raises(InsarError, match="ROCm"):
        iu.stitch_logits(lg.cpu(), origins, 600, 700, T, 32)
    assert trained_unet.training


# ---- one scratch cache for every scene tool ---------------------------------------------------------------------------------
class _SignNet(torch.nn.Module):
    """Class 1 wherever the (normalised) scene is positive; one parameter, so that the predictor finds its device."""

    def __init__(self):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(4.0))

    def forward(self, x):
        return torch.cat([torch.zeros_like(x), self.gain * x], dim=1)


def _same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, torch.Tensor):
        assert _bitwise(a, b), what
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert (a == b).all() if a.dtype == object else np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what
    else:
        assert a == b or (a != a and b != b), what


def test_release_empties_the_one_scratch_cache(dev):
    """A ragged 96 x 80 scene (tile 64, overlap 16: two tiles each way) through every tool detect and evaluate can chain.
    `release()` used to forget the split, skeleton and outline scratch; scratch rebuilt after it gives the same tables."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import regions, score
    H, W = 96, 80
    yy, xx = np.mgrid[:H, :W]
    discs = [(30, 24, 13), (30, 46, 13), (70, 60, 9), (80, 12, 6)]           # the first two touch: one region, two pieces
    inside = np.zeros((H, W), dtype=bool)
    for cy, cx, r in discs:
        inside |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    scene = np.where(inside, 1.0, -1.0).astype(np.float32)
    gt = np.roll(inside, 2, axis=1).astype(np.uint8)
    gt[:3] = 255
    pred = iu.ScenePredictor(_SignNet().to(dev), tile=64, overlap=16, batch=3, num_classes=2)
    kw = dict(outlines=True, simplify=1.0, skeletons=True, split=True, measure={"input": "input"})
    first = pred.detect(scene, **kw)
    assert first["count"] >= 4 and first["split_converged"] and (first["mask"].cpu().numpy() == inside).all()
    ev = pred.evaluate(scene, gt, boundary_distance=2)
    assert ev["score"]["overall"]["tp"] == 3 and ev["score"]["boundary"]["distance"] == 2
    held = {cls for cls, _, _ in pred._cache}
    assert held == {regions.RegionScratch, iu.SplitScratch, iu.OutlineScratch, iu.SkeletonScratch, iu.ZonalScratch,
                    score.OverlapScratch, iu.DistanceScratch}
    assert len(pred._cache) == len(held) and all(d == dev for _, _, d in pred._cache)
    pred.release()
    assert not pred._cache and not pred._geom and not pred._tiles
    again = pred.detect(scene, **kw)
    assert len(pred._cache) == 5
    for k in ("labels", "regions", "count", "mask_clean", "outlines", "skeleton", "stats", "split_rounds"):
        _same(first[k], again[k], k)
