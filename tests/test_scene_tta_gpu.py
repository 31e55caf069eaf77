"""GPU: test-time augmentation in ScenePredictor(tta=...). The stitched probabilities are held against the float64
stitch oracle of tests/test_scene_host.py fed with every op's expected logits (the numpy D4 oracle of tests/augment_ref.py
around the stub net's own function), at the tolerance tests/test_scene_gpu.py uses against the same oracle: 3e-6 absolute on
probabilities in [0, 1]. The stub's logits are a handful of exact or once-rounded float32 operations, restated in numpy."""
import numpy as np
import pytest
import torch

from tests import augment_ref as ref
from tests.test_scene_host import stitch_oracle

pytestmark = pytest.mark.gpu
PROB_TOL = 3e-6
T, OVERLAP, BATCH, K = 32, 8, 3, 2
H, W = 80, 112


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _ramp():
    """float32 [K, T, T]: a fixed, asymmetric function of the position in the tile (no flip or transpose leaves it alone)."""
    i, j = np.meshgrid(np.arange(T, dtype=np.float32), np.arange(T, dtype=np.float32), indexing="ij")
    return np.stack([0.5 + (2 * i + j) / np.float32(64), 1.5 - (i + 3 * j) / np.float32(128)]).astype(np.float32)


class Stub(torch.nn.Module):
    """logits[k] = f_k(x) * ramp[k] with f pointwise: NOT equivariant under D4 unless the ramp is constant."""

    def __init__(self, ramp: np.ndarray):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(1.5))
        self.register_buffer("ramp", torch.from_numpy(ramp))

    def forward(self, x):
        v = x[:, 0]
        return torch.stack([self.w * v, v * v - 0.5], dim=1) * self.ramp


def _stub_numpy(tiles: np.ndarray, ramp: np.ndarray) -> np.ndarray:
    """The stub on float32 tiles [n, T, T] -> [n, K, T, T], the same float32 operations."""
    f0 = np.float32(1.5) * tiles
    f1 = (tiles * tiles).astype(np.float32) - np.float32(0.5)
    return (np.stack([f0, f1], axis=1) * ramp).astype(np.float32)


@pytest.fixture(scope="module")
def scene():
    return np.random.default_rng(77).uniform(-1, 1, size=(H, W)).astype(np.float32)


def _expected_logits(scene, origins, ramp, tta):
    tiles = np.stack([scene[y:y + T, x:x + T] for y, x in origins])
    out = []
    for op in range(tta):
        seen = np.ascontiguousarray(ref.d4(tiles, op))                        # what the net is shown
        out.append(np.ascontiguousarray(ref.d4(_stub_numpy(seen, ramp), ref.INVERSE[op])))      # brought back
    return np.concatenate(out), np.concatenate([origins] * tta)


@pytest.mark.parametrize("tta", [2, 4, 8])
def test_tta_is_the_stitch_of_every_ops_logits(dev, scene, tta):
    import insar_unet_ca_amd as iu
    ramp = _ramp()
    pred = iu.ScenePredictor(Stub(ramp).to(dev), tile=T, overlap=OVERLAP, batch=BATCH, num_classes=K, tta=tta)
    out = pred.predict(scene, return_prob=True)
    origins = iu.plan_tiles(H, W, T, OVERLAP)
    assert len(origins) > BATCH                                               # several batches
    lg, rep = _expected_logits(scene, origins, ramp, tta)
    want, wsum = stitch_oracle(lg, rep, H, W, T, OVERLAP)
    assert (wsum > 0).all()
    prob = out["prob"].cpu().numpy()
    err = np.abs(prob - want).max()
    # how far the answer is from the un-augmented one: the test would be blind if this were inside the tolerance
    plain = stitch_oracle(*_expected_logits(scene, origins, ramp, 1), H, W, T, OVERLAP)[0]
    print(f"tta={tta}: prob err {err:.2e}; distance to the tta=1 answer {np.abs(want - plain).max():.2e}")
    assert np.abs(want - plain).max() > 1e-2
    assert err <= PROB_TOL
    assert np.abs(out["conf"].cpu().numpy() - want.max(axis=0)).max() <= PROB_TOL
    assert out["mask"].dtype == torch.uint8 and out["mask"].shape == (H, W)


def test_tta_of_an_equivariant_net_changes_nothing(dev, scene):
    """A pointwise net commutes with every op, so each op's logits come back as the plain ones: tta = 8 equals tta = 1
    within the tolerance. A wrong inverse op leaves the logits flipped or rotated and cannot pass."""
    import insar_unet_ca_amd as iu
    net = Stub(np.ones((K, T, T), dtype=np.float32)).to(dev)
    kw = dict(tile=T, overlap=OVERLAP, batch=BATCH, num_classes=K)
    one = iu.ScenePredictor(net, **kw).predict(scene, return_prob=True)
    eight = iu.ScenePredictor(net, tta=8, **kw).predict(scene, return_prob=True)
    err = float((one["prob"] - eight["prob"]).abs().max())
    print(f"equivariant stub: |tta 8 - tta 1| {err:.2e}")
    assert err <= PROB_TOL


def test_tta_1_is_the_default_bit_for_bit_and_tta_4_repeats(dev, scene):
    import insar_unet_ca_amd as iu
    net = Stub(_ramp()).to(dev)
    kw = dict(tile=T, overlap=OVERLAP, batch=BATCH, num_classes=K)
    base = iu.ScenePredictor(net, **kw).predict(scene, return_prob=True)
    one = iu.ScenePredictor(net, tta=1, **kw)
    got = one.predict(scene, return_prob=True)
    assert one._tta == {}                                                   # nothing of the TTA path was set up
    for k in ("prob", "conf", "mask"):
        assert got[k].dtype == base[k].dtype and torch.equal(got[k], base[k]), k
    four = iu.ScenePredictor(net, tta=4, **kw)
    a = four.predict(scene, return_prob=True)
    b = four.predict(scene, return_prob=True)
    c = iu.predict_scene(net, scene, return_prob=True, tta=4, **kw)
    d = iu.detect_scene(net, scene, return_prob=True, tta=4, min_area=1, **kw)
    for k in ("prob", "conf", "mask"):
        assert a[k].data_ptr() != b[k].data_ptr()
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) and torch.equal(a[k], d[k]), k
    assert not torch.equal(a["prob"], base["prob"])


def test_tta_8_on_a_real_unet(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).train()
    scene = np.random.default_rng(5).integers(0, 256, size=(64, 64), dtype=np.uint8)
    pred = iu.ScenePredictor(net, tile=32, overlap=8, batch=4, num_classes=2, tta=8)
    out = pred.predict(scene, return_prob=True)
    assert net.training
    assert out["prob"].shape == (2, 64, 64) and out["prob"].dtype == torch.float32
    assert out["mask"].shape == (64, 64) and out["mask"].dtype == torch.uint8
    assert out["conf"].shape == (64, 64) and out["conf"].dtype == torch.float32
    assert bool(torch.isfinite(out["prob"]).all())
    assert float((out["prob"].sum(0) - 1.0).abs().max()) <= 1e-5
    assert len(pred._tta) == 1 and len(pred._geom) == 1
    pred.release()
    assert pred._tta == {} and pred._geom == {} and pred._tiles == {}
