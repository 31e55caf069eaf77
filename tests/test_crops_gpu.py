"""GPU: csrc/crops.hip (insar_crops_cells / _sat / _draw / _gather), CropIndex and SceneCrops against the numpy restatement in
tests/crops_ref.py. Every comparison is bitwise: table, origins, info, images (through their int32 view) and masks."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import crops_ref as ref

pytestmark = pytest.mark.gpu
TILES = (16, 32, 64)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _same_f32(t: torch.Tensor, want: np.ndarray) -> bool:
    got = t.detach().cpu().numpy()
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def _same_int(t: torch.Tensor, want: np.ndarray) -> bool:
    got = t.detach().cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def random_labels(H, W, K, seed):
    """Mostly class 0 with patches of the other classes, stray labels >= K and void runs."""
    rng = np.random.default_rng(seed)
    lab = rng.choice(np.array(list(range(K)) + [K, 77, 255], dtype=np.uint8), size=(H, W),
                     p=np.array([8.0] + [1.0] * (K - 1) + [0.3, 0.3, 1.0]) / (8.0 + K - 1 + 1.6))
    lab[H // 4:H // 2, W // 5:W // 2] = K - 1
    lab[:H // 6, -W // 3:] = 255
    return lab


def random_scene(H, W, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    return rng.standard_normal((H, W)).astype(np.float32)


# shape, cell: the last is filled with class 1 (counts up to 4.2 M in int32); the first four are the issue's, the rest add the
# 16-byte path at every cell size it covers, a cell size outside it, and a row pitch that is a multiple of 16 at cell 1
SHAPES = [((300, 517), 1), ((1030, 77), 1), ((203, 333), 8), ((64, 64), 8), ((2048, 2048), 1),
          ((48, 80), 2), ((96, 112), 4), ((64, 96), 16), ((50, 70), 3), ((70, 64), 1)]
_CASES: dict = {}


def case(shape, g, K):
    """(labels, the oracle's cell table, the oracle's summed table), computed once per case; no test writes to them."""
    key = (shape, g, K)
    if key not in _CASES:
        lab = np.ones(shape, dtype=np.uint8) if shape == (2048, 2048) else random_labels(*shape, K, seed=shape[0] + g + K)
        _CASES[key] = (lab, ref.cell_table(lab, K, g), ref.sat(lab, K, g))
    return _CASES[key]


# ---- the table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("shape, g", SHAPES)
def test_cells_and_sat_equal_the_oracle(dev, shape, g, K):
    from insar_unet_ca_amd import _lib
    lab, want_cells, want_sat = case(shape, g, K)
    H, W = shape
    Hc, Wc = H // g, W // g
    d_lab = torch.from_numpy(lab).to(dev)
    numel = (K + 1) * (Hc + 1) * (Wc + 1)
    buf = torch.full((numel + 128,), -7, dtype=torch.int32, device=dev)
    table = buf[64:64 + numel]
    _lib.call("insar_crops_cells", d_lab.data_ptr(), H, W, K, g, table.data_ptr(), _lib.stream_ptr())
    assert _same_int(table.view(K + 1, Hc + 1, Wc + 1), want_cells)
    _lib.call("insar_crops_sat", table.data_ptr(), K, Hc, Wc, _lib.stream_ptr())
    got = buf.cpu().numpy()
    assert np.array_equal(got[64:64 + numel].reshape(K + 1, Hc + 1, Wc + 1), want_sat)
    assert (got[:64] == -7).all() and (got[64 + numel:] == -7).all()          # nothing outside the table
    if shape == (2048, 2048):
        assert want_sat[1, Hc, Wc] == H * W and want_sat[0, Hc, Wc] == 0


def test_cells_from_a_misaligned_map_take_the_byte_path(dev):
    """W % 16 == 0 and cell 8, but the map starts 3 bytes into its buffer: no error, the same table."""
    from insar_unet_ca_amd import _lib
    lab, want_cells, _ = case((64, 64), 8, 2)
    flat = torch.zeros(64 * 64 + 16, dtype=torch.uint8, device=dev)
    flat[3:3 + 64 * 64] = torch.from_numpy(lab).to(dev).flatten()
    table = torch.empty(3, 9, 9, dtype=torch.int32, device=dev)
    _lib.call("insar_crops_cells", flat.data_ptr() + 3, 64, 64, 2, 8, table.data_ptr(), _lib.stream_ptr())
    assert _same_int(table, want_cells)


def test_crop_index(dev):
    import insar_unet_ca_amd as iu
    lab, _, want = case((203, 333), 8, 5)
    idx = iu.CropIndex(lab, 5, cell=8, device=dev)
    assert _same_int(idx.table, want) and idx.nbytes == want.size * 4 and (idx.Hc, idx.Wc) == (25, 41)
    assert idx.candidates(32) == 22 * 38
    origins = np.array([[0, 0], [8, 296], [168, 0], [96, 104]], dtype=np.int32)
    got = idx.counts(torch.from_numpy(origins).to(dev), 32)
    assert got.is_cuda and _same_int(got, ref.counts(want, origins, 32, 8))
    for (y, x), row in zip(origins, got.cpu().numpy()):
        box = lab[y:y + 32, x:x + 32]
        assert row.tolist() == [int((box == p).sum()) for p in range(5)] + [int((box >= 5).sum())]
    px = idx.class_pixels()
    assert px.is_cuda and px.dtype == torch.int64 and px.cpu().tolist() == [int((lab[:200, :328] == p).sum()) for p in range(5)]
    w = iu.class_weights(px.cpu())
    assert w.shape == (5,) and bool((w > 0).all())


# ---- draw and gather on the issue's shapes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("shape, g", SHAPES[:5])
def test_draw_and_gather_equal_the_oracle(dev, shape, g, K):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import crops
    lab, _, table = case(shape, g, K)
    H, W = shape
    scene = random_scene(H, W, np.uint8, seed=H)
    d_scene, idx = torch.from_numpy(scene).to(dev), iu.CropIndex(lab, K, cell=g, device=dev)
    cum = crops.cumulative([1.0] * K)
    for T in TILES:
        if T > min(H, W):
            continue
        key, n = crops.batch_key(T, 0, K), 6
        min_count, max_void = crops.count_limits(T, 0.05, 0.25)
        origins, info = iu.draw_crops(idx, key, n, T, cum, min_count, max_void, 16)
        want_o, want_i = ref.draw(key, n, K, 16, cum, min_count, max_void, T, g, H, W, table)
        assert _same_int(origins, want_o) and _same_int(info, want_i)
        if shape == (64, 64) and T == 64:
            assert (want_o == 0).all()                                          # ny = nx = 1: every try gives the same origin
        images, masks = iu.gather_crops(d_scene, idx.labels, origins, T)
        want_x, want_m = ref.gather(scene, lab, want_o, T)
        assert _same_f32(images, want_x) and _same_int(masks, want_m)


# ---- the draw's rules --------------------------------------------------------------------------------------------------------
def blob_scene(H, W, frac=0.02):
    lab = np.zeros((H, W), dtype=np.uint8)
    side = int(round((frac * H * W) ** 0.5))
    lab[H // 3:H // 3 + side, W // 2:W // 2 + side] = 1
    return lab


@pytest.mark.parametrize("tries", [1, 16, 64])
def test_draw_rules(dev, tries):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import crops
    H, W, g, T, n = 256, 320, 8, 32, 40
    min_count, max_void = crops.count_limits(T, 0.01, 0.5)
    # one blob of class 1 on about 2 % of the scene: both classes asked for
    lab = blob_scene(H, W)
    assert 0.015 < (lab == 1).mean() < 0.025
    idx, table = iu.CropIndex(lab, 2, cell=g, device=dev), ref.sat(lab, 2, g)
    cum = crops.cumulative([1.0, 1.0])
    key = crops.batch_key(9, 0, tries)
    origins, info = iu.draw_crops(idx, key, n, T, cum, min_count, max_void, tries)
    want_o, want_i = ref.draw(key, n, 2, tries, cum, min_count, max_void, T, g, H, W, table)
    assert _same_int(origins, want_o) and _same_int(info, want_i)
    # follows from the rule, no statistic: an accepted try holds at least min_count target pixels and at most max_void void ones
    got = idx.counts(origins, T).cpu().numpy()
    i = info.cpu().numpy()
    ok = i[:, 1] >= 0
    assert (got[ok, i[ok, 0]] >= min_count).all() and (got[ok, 2] <= max_void).all() and (i[:, 1] < tries).all()
    assert (got[np.arange(n), i[:, 0]] == i[:, 2]).all() and (got[:, 2] == i[:, 3]).all()
    assert set(i[:, 0].tolist()) == {0, 1}
    if tries == 64:
        assert ok[i[:, 0] == 1].any()                                           # 64 tries find the blob for some sample
    # a class listed in class_probs but absent from the scene: the fallback, info says -1
    idx3, table3 = iu.CropIndex(lab, 3, cell=g, device=dev), ref.sat(lab, 3, g)
    cum3 = crops.cumulative([0.0, 0.0, 1.0])
    origins, info = iu.draw_crops(idx3, key, n, T, cum3, min_count, max_void, tries)
    want_o, want_i = ref.draw(key, n, 3, tries, cum3, min_count, max_void, T, g, H, W, table3)
    assert _same_int(origins, want_o) and _same_int(info, want_i)
    assert (want_i[:, 0] == 2).all() and (want_i[:, 1] == -1).all() and (want_i[:, 2] == 0).all()
    # an all-void scene: no try is within the cap, the fewest-void rule (all equal: try 0)
    void = np.full((H, W), 255, dtype=np.uint8)
    void[100:120, 60:200] = 0                                                   # fewer void pixels around here, never none
    idxv, tablev = iu.CropIndex(void, 2, cell=g, device=dev), ref.sat(void, 2, g)
    origins, info = iu.draw_crops(idxv, key, n, T, cum, min_count, 0, tries)
    want_o, want_i = ref.draw(key, n, 2, tries, cum, min_count, 0, T, g, H, W, tablev)
    assert _same_int(origins, want_o) and _same_int(info, want_i) and (want_i[:, 1] == -1).all() and (want_i[:, 3] > 0).all()


def test_draw_writes_only_its_rows(dev):
    from insar_unet_ca_amd import _lib, crops
    lab, _, table = case((203, 333), 8, 2)
    d_table = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    n, T = 7, 32
    o = torch.full((n + 2, 2), -7, dtype=torch.int32, device=dev)
    i = torch.full((n + 2, 4), -7, dtype=torch.int32, device=dev)
    cum = crops.cumulative([1.0, 3.0])
    _lib.call("insar_crops_draw", 12345, n, 2, 16, cum.ctypes.data_as(C.c_void_p), 20, 300, T, 8, 203, 333, d_table.data_ptr(),
              o[1:].data_ptr(), i[1:].data_ptr(), _lib.stream_ptr())
    want_o, want_i = ref.draw(12345, n, 2, 16, cum, 20, 300, T, 8, 203, 333, table)
    go, gi = o.cpu().numpy(), i.cpu().numpy()
    assert np.array_equal(go[1:n + 1], want_o) and np.array_equal(gi[1:n + 1], want_i)
    assert (go[0] == -7).all() and (go[n + 1] == -7).all() and (gi[0] == -7).all() and (gi[n + 1] == -7).all()


# ---- gather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("mask_dtype", [torch.int64, torch.uint8])
def test_gather_equals_gather_tiles_and_the_oracle(dev, scene_dtype, mask_dtype):
    import insar_unet_ca_amd as iu
    H, W, T = 203, 333, 32
    scene, lab = random_scene(H, W, scene_dtype, seed=4), random_labels(H, W, 3, seed=6)
    origins = np.array([[0, 0], [171, 301], [8, 13], [77, 1], [5, 300], [171, 0], [100, 150]], dtype=np.int32)      # unaligned ones too
    d_scene, d_lab, d_o = torch.from_numpy(scene).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(origins).to(dev)
    images, masks = iu.gather_crops(d_scene, d_lab, d_o, T, mask_dtype)
    want_x, want_m = ref.gather(scene, lab, origins, T, np.int64 if mask_dtype == torch.int64 else np.uint8)
    assert _same_f32(images, want_x) and _same_int(masks, want_m)
    tiles = iu.gather_tiles(d_scene, d_o, T)
    assert torch.equal(images.view(torch.int32), tiles.view(torch.int32))
    only_x, none_m = iu.gather_crops(d_scene, None, d_o, T)
    none_x, only_m = iu.gather_crops(None, d_lab, d_o, T, mask_dtype)
    assert none_m is None and none_x is None and torch.equal(only_x.view(torch.int32), tiles.view(torch.int32)) and torch.equal(only_m, masks)


def test_gather_writes_only_its_tiles(dev):
    from insar_unet_ca_amd import _lib
    H, W, T, n = 70, 64, 16, 3
    scene, lab = random_scene(H, W, np.uint8, seed=1), random_labels(H, W, 2, seed=2)
    origins = np.array([[0, 0], [54, 48], [33, 7]], dtype=np.int32)
    d_scene, d_lab, d_o = torch.from_numpy(scene).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(origins).to(dev)
    x = torch.full((n * T * T + 128,), -7.0, dtype=torch.float32, device=dev)
    m = torch.full((n * T * T + 128,), -7, dtype=torch.int64, device=dev)
    _lib.call("insar_crops_gather", d_scene.data_ptr(), _lib.SCENE_U8, d_lab.data_ptr(), H, W, d_o.data_ptr(), n, T,
              x[64:].data_ptr(), m[64:].data_ptr(), _lib.AUG_MASK_I64, _lib.stream_ptr())
    want_x, want_m = ref.gather(scene, lab, origins, T)
    gx, gm = x.cpu().numpy(), m.cpu().numpy()
    assert np.array_equal(gx[64:-64].view(np.int32), want_x.reshape(-1).view(np.int32)) and np.array_equal(gm[64:-64], want_m.reshape(-1))
    assert (gx[:64] == -7).all() and (gx[-64:] == -7).all() and (gm[:64] == -7).all() and (gm[-64:] == -7).all()


# ---- SceneCrops --------------------------------------------------------------------------------------------------------------
def two_scenes():
    a, b = blob_scene(128, 160), random_labels(96, 200, 2, seed=8)
    return [random_scene(128, 160, np.uint8, seed=1), random_scene(96, 200, np.float32, seed=2)], [a, b]


def make(dev, **kw):
    import insar_unet_ca_amd as iu
    scenes, labels = two_scenes()
    args = dict(tile=32, batch=4, steps_per_epoch=5, num_classes=2, tries=16, cell=8, seed=3, rank=1, device=dev)
    args.update(kw)
    return iu.SceneCrops(scenes, labels, **args), scenes, labels


def test_scene_crops_follow_the_oracle_and_repeat(dev):
    from insar_unet_ca_amd import crops
    a, scenes, labels = make(dev)
    b, _, _ = make(dev)
    assert len(a) == 5 and a.class_probs == [1.0, 1.0] and (a.min_count, a.max_void) == (11, 512)
    tables = [ref.sat(lb, 2, 8) for lb in labels]
    used = set()
    for step, ((xa, ma), (xb, mb)) in enumerate(zip(a, b)):
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(ma, mb)
        key = crops.batch_key(3, 1, step)
        i = crops.pick_scene(key, a.candidates)
        used.add(i)
        H, W = labels[i].shape
        want_o, want_i = ref.draw(key, 4, 2, 16, a.cum, 11, 512, 32, 8, H, W, tables[i])
        want_x, want_m = ref.gather(scenes[i], labels[i], want_o, 32)
        assert a.last_scene == i and _same_int(a.last_origins, want_o) and _same_int(a.last_info, want_i)
        assert _same_f32(xa, want_x) and _same_int(ma, want_m) and xa.is_cuda and ma.dtype == torch.int64
    assert a.step == 5 and a.candidates == [13 * 17, 9 * 22] and used <= {0, 1}
    u8, _, _ = make(dev, mask_dtype=torch.uint8)
    x8, m8 = u8.next_batch()
    a.load_state_dict(dict(a.state_dict(), step=0))
    x0, m0 = a.next_batch()
    assert m8.dtype == torch.uint8 and torch.equal(m8.long(), m0) and torch.equal(x8, x0)
    other, _, _ = make(dev, rank=2)
    other.next_batch()
    assert not torch.equal(other.last_origins, u8.last_origins) or other.last_scene != u8.last_scene


def test_scene_crops_resume_from_a_state(dev):
    import insar_unet_ca_amd as iu
    aug = lambda: iu.Augment(seed=5, rank=1, ops="d4", gain=(0.8, 1.25), bias=(-0.1, 0.1), noise_sigma=(0.0, 0.1))
    a, _, _ = make(dev, augment=aug())
    it = iter(a)
    next(it), next(it)
    state = a.state_dict()
    assert state["step"] == 2 and state["seed"] == 3 and state["rank"] == 1 and state["augment"]["step"] == 2
    b, _, _ = make(dev, augment=aug())
    b.load_state_dict(state)
    for _ in range(3):
        (xa, ma), (xb, mb) = a.next_batch(), b.next_batch()
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(ma, mb)
    c, _, _ = make(dev, tile=64)
    with pytest.raises(iu.InsarError, match="config"):
        c.load_state_dict(state)


def test_scene_crops_with_augment_equal_apply_table(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.augment import apply_table
    kw = dict(seed=5, rank=1, ops="d4", gain=(0.8, 1.25), bias=(-0.1, 0.1), noise_sigma=(0.0, 0.1))
    plain, _, _ = make(dev)
    with_aug, _, _ = make(dev, augment=iu.Augment(**kw))
    twin = iu.Augment(**kw)
    for step in range(3):
        x, m = plain.next_batch()
        xa, ma = with_aug.next_batch()
        want_x, want_m = apply_table(x, m, twin.draw(4, dev, step=step), twin.noise_seed(step))
        assert torch.equal(xa.view(torch.int32), want_x.view(torch.int32)) and torch.equal(ma, want_m)
        assert not torch.equal(xa, x)


def test_no_read_back_after_construction(dev, monkeypatch):
    """Through the API: building a SceneCrops reads the class totals back once; drawing batches, counts() and class_pixels()
    never bring a tensor to the host."""
    import insar_unet_ca_amd as iu
    calls = []
    for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda orig, name: lambda self, *a, **k: (calls.append(name), orig(self, *a, **k))[1])(orig, name))
    crops, _, _ = make(dev, augment=iu.Augment(seed=1))
    assert calls.count("cpu") == 1
    del calls[:]
    for x, m in crops:
        pass
    crops.indices[crops.last_scene].counts(crops.last_origins, 32)
    crops.indices[0].class_pixels()
    assert calls == [] and crops.last_info.is_cuda
    explicit, _, _ = make(dev, class_probs=[0.5, 0.5])                           # nothing to find out: no read-back at all
    explicit.next_batch()
    assert calls == []


def test_train_model_takes_scene_crops(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(0)
    lab = blob_scene(128, 128, frac=0.1)
    scene = (random_scene(128, 128, np.uint8, seed=3) // 2 + lab * 100).astype(np.uint8)
    crops = iu.SceneCrops(scene, lab, tile=32, batch=2, steps_per_epoch=3, num_classes=2, cell=8, seed=0, device=dev,
                          augment=iu.Augment(seed=0, ops="flips"))
    net = iu.UNet(1, 2, True).to(dev)
    hist = iu.train_model(net, crops, None, iu.CrossEntropyLoss(ignore_index=255), iu.Adam(net.parameters(), lr=1e-3), dev,
                          num_epochs=1, verbose=False)
    assert len(hist) == 1 and np.isfinite(hist[0]["train_loss"]) and crops.step == 3
    assert all(np.isfinite(v) for v in hist[0].values())
