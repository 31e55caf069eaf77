"""CPU-only: the oracle of tests/crops_ref.py against brute-force counting, the properties of the draw rule, the host
arithmetic of insar_unet_ca_amd/crops.py (keys, scene choice, limits, state), and the argument validation of the four C entry
points of csrc/crops.hip (no device is touched)."""
import ctypes as C

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _lib, augment, crops
from insar_unet_ca_amd._lib import InsarError
from tests import crops_ref as ref


def random_labels(H, W, K, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array(list(range(K)) + [K, 200, 255], dtype=np.uint8), size=(H, W))


# ---- the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W, K, g", [(37, 53, 2, 1), (37, 53, 5, 4), (40, 64, 3, 8), (19, 23, 8, 3)])
def test_rectangle_counts_equal_brute_force(H, W, K, g):
    lab = random_labels(H, W, K, seed=H * W + g)
    table = ref.sat(lab, K, g)
    Hc, Wc = H // g, W // g
    assert table.shape == (K + 1, Hc + 1, Wc + 1) and (table[:, 0] == 0).all() and (table[:, :, 0] == 0).all()
    rng = np.random.default_rng(5)
    for _ in range(40):
        n = int(rng.integers(1, min(Hc, Wc) + 1))
        a0, b0 = int(rng.integers(0, Hc - n + 1)), int(rng.integers(0, Wc - n + 1))
        box = lab[a0 * g:(a0 + n) * g, b0 * g:(b0 + n) * g]
        for p in range(K):
            assert ref.rect(table, p, a0, b0, n) == int((box == p).sum())
        assert ref.rect(table, K, a0, b0, n) == int((box >= K).sum())            # 255 and every other label >= K
    # the corner holds the whole cell area; the ragged edges belong to no cell
    assert int(table[:, Hc, Wc].astype(np.int64).sum()) == Hc * g * Wc * g
    origins = np.array([[0, 0], [g, 2 * g]], dtype=np.int32)
    T = g * min(3, Hc - 1, Wc - 2)
    got = ref.counts(table, origins, T, g)
    for (y, x), row in zip(origins, got):
        box = lab[y:y + T, x:x + T]
        assert row.tolist() == [int((box == p).sum()) for p in range(K)] + [int((box >= K).sum())]


def blob_scene(H, W, frac=0.02):
    lab = np.zeros((H, W), dtype=np.uint8)
    side = int(round((frac * H * W) ** 0.5))
    lab[H // 3:H // 3 + side, W // 2:W // 2 + side] = 1
    return lab


def test_origins_are_cell_multiples_inside_the_scene_and_reach_both_ends():
    H, W, K, g, T = 203, 333, 2, 8, 32
    lab = blob_scene(H, W)
    table = ref.sat(lab, K, g)
    cum = crops.cumulative([1.0, 1.0])
    ny = H // g - T // g + 1
    seen = set()
    for step in range(12):
        o, info = ref.draw(crops.batch_key(3, 0, step), 16, K, 16, cum, 10, T * T // 2, T, g, H, W, table)
        assert (o % g == 0).all() and (o >= 0).all() and (o[:, 0] + T <= H).all() and (o[:, 1] + T <= W).all()
        assert set(info[:, 0].tolist()) <= {0, 1} and ((info[:, 1] >= -1) & (info[:, 1] < 16)).all()
        got = ref.counts(table, o, T, g)
        assert (got[np.arange(16), info[:, 0]] == info[:, 2]).all() and (got[:, K] == info[:, 3]).all()
        ok = info[:, 1] >= 0
        assert (info[ok, 2] >= 10).all()
    # the multiply-shift reaches both ends of 0 .. ny - 1: every try of many samples, as the rule forms it
    key = crops.batch_key(0, 0, 0)
    for i in range(4000):
        seen.add(((augment.aug_hash64(key, i) >> 32) * ny) >> 32)
    assert min(seen) == 0 and max(seen) == ny - 1 and len(seen) == ny


def test_draw_is_deterministic_and_ranks_differ():
    H, W, K, g, T = 96, 128, 3, 4, 16
    lab = random_labels(H, W, K, seed=1)
    table = ref.sat(lab, K, g)
    cum = crops.cumulative([0.2, 0.3, 0.5])
    args = (8, K, 16, cum, 40, 128, T, g, H, W, table)
    a = ref.draw(crops.batch_key(7, 0, 4), *args)
    b = ref.draw(crops.batch_key(7, 0, 4), *args)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = ref.draw(crops.batch_key(7, 1, 4), *args)
    d = ref.draw(crops.batch_key(7, 0, 5), *args)
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[0], d[0])


def test_fallback_rules_by_hand():
    H = W = 64
    K, g, T = 2, 8, 16
    cum = np.array([0.0, 1.0], dtype=np.float32)                       # the target is always class 1
    key = crops.batch_key(1, 0, 0)
    # class 1 absent: no try is accepted, every try has 0 target pixels: the tie goes to try 0
    table = ref.sat(np.zeros((H, W), dtype=np.uint8), K, g)
    o, info = ref.draw(key, 5, K, 16, cum, 1, T * T, T, g, H, W, table)
    assert (info[:, 0] == 1).all() and (info[:, 1] == -1).all() and (info[:, 2] == 0).all()
    for s in range(5):
        r = augment.aug_hash64(key, 65 * s + 1)
        assert o[s].tolist() == [(((r >> 32) * 7) >> 32) * g, (((r & 0xffffffff) * 7) >> 32) * g]
    # all void, cap 0: no try is within the cap, all have T * T void pixels: try 0 again, and info says so
    table = ref.sat(np.full((H, W), 255, dtype=np.uint8), K, g)
    o2, info = ref.draw(key, 5, K, 16, cum, 1, 0, T, g, H, W, table)
    assert np.array_equal(o, o2) and (info[:, 1] == -1).all() and (info[:, 3] == T * T).all()
    # a void left half with cap 0: the chosen try has the fewest void pixels of its 16 tries
    lab = np.zeros((H, W), dtype=np.uint8)
    lab[:, :32] = 255
    table = ref.sat(lab, K, g)
    o, info = ref.draw(key, 8, K, 16, cum, 1, T * T // 4, T, g, H, W, table)
    for s in range(8):
        tries = [augment.aug_hash64(key, 65 * s + 1 + t) for t in range(16)]
        voids = [ref.rect(table, K, ((r >> 32) * 7) >> 32, ((r & 0xffffffff) * 7) >> 32, 2) for r in tries]
        if min(voids) <= T * T // 4:
            assert info[s, 3] == voids[[v <= T * T // 4 for v in voids].index(True)]      # all have 0 target pixels: first within the cap
        else:
            assert info[s, 3] == min(voids)


# ---- host arithmetic of crops.py ------------------------------------------------------------------------------------------
def test_keys_limits_and_scene_choice():
    assert crops.CROP_STREAM != augment.NOISE_STREAM and crops.SCENE_STREAM not in (crops.CROP_STREAM, augment.NOISE_STREAM)
    k = crops.batch_key(5, 2, 9)
    assert k == augment.aug_hash64(augment.aug_hash64(5, 2) ^ crops.CROP_STREAM, 9) and 0 <= k < 1 << 64
    assert k != augment.Augment(seed=5, rank=2).noise_seed(9)
    assert crops.count_limits(256, 0.01, 0.5) == (656, 32768) and crops.count_limits(32, 0.0, 1.0) == (0, 1024)
    assert crops.count_limits(16, 0.01, 0.999) == (3, 255)
    for bad in ((-0.1, 0.5), (0.1, 1.5), ("a", 0.5)):
        with pytest.raises(InsarError, match="fraction"):
            crops.count_limits(32, *bad)
    cum = crops.cumulative([1, 0, 3])
    assert cum.dtype == np.float32 and cum.tolist() == [0.25, 0.25, 1.0]
    for bad in ([0, 0], [-1, 2], [], [float("nan"), 1]):
        with pytest.raises(InsarError, match="class_probs"):
            crops.cumulative(bad)
    picks = [crops.pick_scene(crops.batch_key(0, 0, s), [100, 300]) for s in range(400)]
    assert set(picks) == {0, 1} and 60 <= picks.count(0) <= 140         # 100 expected, sd 8.7
    assert all(crops.pick_scene(crops.batch_key(0, 0, s), [0, 7, 0]) == 1 for s in range(50))
    with pytest.raises(InsarError, match="candidate"):
        crops.pick_scene(1, [0, 0])


def test_state_round_trips_and_is_checked():
    cfg = {"tile": 32, "batch": 4, "class_probs": [1.0, 1.0]}
    st = crops.make_state(11, 3, 17, cfg)
    assert st == {"seed": 11, "rank": 3, "step": 17, "config": cfg}
    assert crops.check_state(st) == (11, 3, 17, cfg)
    import json
    assert crops.check_state(json.loads(json.dumps(st))) == (11, 3, 17, cfg)
    for bad in ({}, {"seed": 1, "rank": 0, "step": 0}, {"seed": "x", "rank": 0, "step": 0, "config": {}},
                {"seed": 1, "rank": 0, "step": -1, "config": {}}, {"seed": 1, "rank": 0, "step": 0, "config": 3}):
        with pytest.raises(InsarError, match="load_state_dict"):
            crops.check_state(bad)


def test_python_arguments_are_refused_before_any_launch():
    lab = np.zeros((64, 64), dtype=np.uint8)
    sc = np.zeros((64, 64), dtype=np.float32)
    with pytest.raises(InsarError, match="num_classes"):
        iu.SceneCrops(sc, lab, tile=32, num_classes=9)
    with pytest.raises(InsarError, match="tries"):
        iu.SceneCrops(sc, lab, tile=32, tries=65)
    with pytest.raises(InsarError, match="tries"):
        iu.SceneCrops(sc, lab, tile=32, tries=0)
    with pytest.raises(InsarError, match="multiple of 4 and of the cell size"):
        iu.SceneCrops(sc, lab, tile=36, cell=8)
    with pytest.raises(InsarError, match="smaller than the tile"):
        iu.SceneCrops(sc, lab, tile=128)
    with pytest.raises(InsarError, match="cell"):
        iu.SceneCrops(sc, lab, tile=32, cell=0)
    with pytest.raises(InsarError, match="one shape"):
        iu.SceneCrops(sc, lab[:32], tile=32)
    with pytest.raises(InsarError, match="two lists"):
        iu.SceneCrops([sc], lab, tile=32)
    with pytest.raises(InsarError, match="mask_dtype"):
        iu.SceneCrops(sc, lab, tile=32, mask_dtype=torch.int32)
    with pytest.raises(InsarError, match="fraction"):
        iu.SceneCrops(sc, lab, tile=32, min_fraction=2.0)
    with pytest.raises(InsarError, match="labels dtype"):
        iu.CropIndex(sc, 2, device="cpu")
    with pytest.raises(InsarError, match="ROCm device"):               # everything else in order: only the device is wrong
        iu.CropIndex(lab, 2, cell=8, device="cpu")
    with pytest.raises(InsarError, match="ROCm"):
        iu.gather_crops(torch.zeros(64, 64), None, torch.zeros(2, 2, dtype=torch.int32), 32)


# ---- the C entry points ---------------------------------------------------------------------------------------------------
def test_c_entry_points_validate_before_the_device():
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    cum = (C.c_float * 8)(*([1.0] * 8))
    call = _lib.call

    def cells(labels=p, H=64, W=64, K=2, g=8, table=p):
        call("insar_crops_cells", labels, H, W, K, g, table, None)

    def sat(table=p, K=2, Hc=8, Wc=8):
        call("insar_crops_sat", table, K, Hc, Wc, None)

    def draw(n=4, K=2, tries=16, cum=cum, T=32, g=8, H=64, W=64, sat=p, origins=p, info=p):
        call("insar_crops_draw", 1, n, K, tries, cum, 10, 100, T, g, H, W, sat, origins, info, None)

    def gather(scene=p, sdt=_lib.SCENE_U8, labels=p, H=64, W=64, origins=p, n=2, T=32, images=p, masks=p, mdt=_lib.AUG_MASK_I64):
        call("insar_crops_gather", scene, sdt, labels, H, W, origins, n, T, images, masks, mdt, None)

    for fn, names in ((cells, ("labels", "table")), (sat, ("table",)), (draw, ("cum", "sat", "origins", "info")),
                      (gather, ("origins",))):
        for name in names:
            with pytest.raises(InsarError, match=rf"null pointer \({name}"):
                fn(**{name: None})
    with pytest.raises(InsarError, match="neither images nor masks"):
        gather(images=None, masks=None)
    with pytest.raises(InsarError, match=r"null pointer \(scene"):
        gather(scene=None)
    with pytest.raises(InsarError, match=r"null pointer \(labels"):
        gather(labels=None)
    for fn in (cells, sat, draw):
        for K in (1, 9):
            with pytest.raises(InsarError, match=rf"num_classes {K} outside 2\.\.8"):
                fn(K=K)
    for fn in (cells, draw):
        for g in (0, -3):
            with pytest.raises(InsarError, match=rf"cell size {g} below 1"):
                fn(g=g)
        with pytest.raises(InsarError, match="2\\^31 pixels or more"):
            fn(H=32768, W=65536)
        with pytest.raises(InsarError, match="empty scene"):
            fn(H=0)
    with pytest.raises(InsarError, match="2\\^31 pixels or more"):
        gather(H=65536, W=32768)
    with pytest.raises(InsarError, match="tile 36 is not a positive multiple of the cell size 8"):
        draw(T=36)
    with pytest.raises(InsarError, match="tile 0 is not a positive multiple"):
        draw(T=0)
    with pytest.raises(InsarError, match="tile 72 above the scene 64 x 80"):
        draw(T=72, W=80)
    with pytest.raises(InsarError, match="tile 72 above the scene 80 x 64"):
        draw(T=72, H=80)
    for tries in (0, 65, -1):
        with pytest.raises(InsarError, match=rf"tries {tries} outside 1\.\.64"):
            draw(tries=tries)
    with pytest.raises(InsarError, match="n = 0"):
        draw(n=0)
    with pytest.raises(InsarError, match="empty table"):
        sat(Hc=0)
    with pytest.raises(InsarError, match="tile 30 is not a positive multiple of 4"):
        gather(T=30)
    with pytest.raises(InsarError, match="tile 128 above the scene"):
        gather(T=128)
    with pytest.raises(InsarError, match="scene dtype 2"):
        gather(sdt=2)
    with pytest.raises(InsarError, match="mask dtype 0"):
        gather(mdt=_lib.AUG_MASK_NONE)
    with pytest.raises(InsarError, match="not 16-byte aligned"):
        gather(images=p + 4)
    with pytest.raises(InsarError, match="not 4-byte aligned"):
        cells(table=p + 2)
    lib = _lib.load()
    assert lib.insar_crops_draw(1, 4, 2, 65, cum, 10, 100, 32, 8, 64, 64, p, p, p, None) == -1005
    assert lib.insar_crops_cells(p, 64, 64, 9, 8, p, None) == -1001


def test_abi_is_additive_and_the_hash_is_unchanged():
    assert _lib.ABI_VERSION == 8 and _lib.load().insar_version() == 8
    for name in ("insar_crops_cells", "insar_crops_sat", "insar_crops_draw", "insar_crops_gather"):
        assert name in _lib.EXPORTED_SYMBOLS
    for name in ("CropIndex", "SceneCrops", "draw_crops", "gather_crops"):
        assert name in iu.__all__ and hasattr(iu, name)
    # splitmix64's finalizer over key + golden * (i + 1): values pinned from the definition
    def splitmix(key, i):
        m = (1 << 64) - 1
        z = (key + 0x9E3779B97F4A7C15 * (i + 1)) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)
    assert augment.aug_hash64(0, 0) == 0xE220A8397B1DCDAF                # splitmix64(seed 0), first output
    for key, i in ((0, 0), (1, 2), ((1 << 64) - 1, 12345), (0x123456789ABCDEF0, 1 << 40)):
        assert augment.aug_hash64(key, i) == splitmix(key, i)
    assert augment.NOISE_STREAM == 0x5851F42D4C957F2D
