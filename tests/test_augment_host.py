"""CPU-only: the numpy oracle of the augmentation (tests/augment_ref.py) pinned against independent facts, the argument
validation of insar_aug_draw / insar_aug_apply through the C ABI (nothing is launched: every refusal comes before the device
is touched), and the host-side checks of Augment and of ScenePredictor(tta=...)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import augment_ref as ref

E_SHAPE, E_DTYPE, E_ARG = -1001, -1002, -1005


# ---- the oracle against independent facts --------------------------------------------------------------------------------
def _plane():
    return np.arange(5 * 5, dtype=np.int64).reshape(5, 5)


def test_op_set_is_the_rot90_family():
    a = _plane()
    family = [np.rot90(a, k) for k in range(4)] + [np.rot90(a.T, k) for k in range(4)]
    ops = [ref.d4(a, op) for op in range(8)]
    for b in ops:
        assert sum(np.array_equal(b, f) for f in family) == 1
    for f in family:
        assert sum(np.array_equal(b, f) for b in ops) == 1
    assert np.array_equal(ref.d4(a, 6), np.rot90(a, 1))
    assert np.array_equal(ref.d4(a, 5), np.rot90(a, 3))
    assert np.array_equal(ref.d4(a, 0), a) and np.array_equal(ref.d4(a, 4), a.T)


def test_inverse_table():
    from insar_unet_ca_amd.augment import D4_INVERSE
    a = _plane()
    assert tuple(D4_INVERSE) == ref.INVERSE == (0, 1, 2, 3, 4, 6, 5, 7)
    for op in range(8):
        assert np.array_equal(ref.d4(ref.d4(a, op), ref.INVERSE[op]), a)
        for other in range(8):
            if other != ref.INVERSE[op]:
                assert not np.array_equal(ref.d4(ref.d4(a, op), other), a)
    # non-square planes keep the four flips
    r = np.arange(12).reshape(3, 4)
    for op in range(4):
        assert ref.d4(r, op).shape == r.shape and np.array_equal(ref.d4(ref.d4(r, op), op), r)


def test_hash_matches_the_python_integer_form():
    from insar_unet_ca_amd.augment import aug_hash64
    for key, i in ((0, 0), (12345, 7), ((1 << 64) - 1, (1 << 40) + 3), (0x9E3779B97F4A7C15, 1 << 63)):
        z = (key + 0x9E3779B97F4A7C15 * (i + 1)) % (1 << 64)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
        want = z ^ (z >> 31)
        assert ref.hash64_int(key, i) == want == aug_hash64(key, i)


def test_uniform_lies_in_the_half_open_unit_interval():
    h = np.array([0, 1, 255, 256, 0x7fffffff, 0xffffffff], dtype=np.uint64)
    u = ref.uniform(h)
    assert u.dtype == np.float32 and u[0] == 0 and u[2] == 0 and u[3] == np.float32(2.0 ** -24)
    assert u.max() == np.float32(1.0 - 2.0 ** -24) and (u >= 0).all() and (u < 1).all()
    u = ref.uniform(ref.hash64(99, np.arange(1 << 16)) >> np.uint64(32))
    assert (u >= 0).all() and (u < 1).all()


def test_noise_is_close_to_unit_normal_and_bounded():
    """N = 2^20: the standard error of the mean is 1e-3 and of the deviation 7e-4; the bounds are five of the former.
    |z| <= 131070 * ZS = 3.4641 for any hash. Measured: mean -0.0014, std 0.9992, max 3.38."""
    z = ref.noise_z(12345, np.arange(1 << 20)).astype(np.float64)
    print(f"noise: mean {z.mean():+.4f}, std {z.std():.4f}, max |z| {np.abs(z).max():.3f}")
    assert abs(z.mean()) < 0.005
    assert abs(z.std() - 1.0) < 0.005
    assert np.abs(z).max() < 3.47
    assert float(np.float32(131070) * ref.ZS) < 3.47
    assert ref.ZS == np.float32(1.0 / np.sqrt((65536.0 ** 2 - 1.0) / 3.0))


def test_every_op_is_drawn():
    """ops_mask = 0xff over 4096 samples: 512 expected per op, deviation 21; 400..620 is over five of them either side."""
    t = ref.draw(ref.key_seed(0, 0), 0, 4096, 0xff, (1, 1), (0, 0), (0, 0))
    counts = np.bincount(t[:, 0], minlength=8)
    print("op counts:", counts.tolist())
    assert counts.sum() == 4096 and counts.min() >= 400 and counts.max() <= 620
    assert (t[:, 1].view(np.float32) == 1).all() and (t[:, 2:] == 0).all()
    # a sparse mask only ever yields its own bits
    t = ref.draw(5, 3, 512, 0x61, (0.5, 2.0), (-1, 1), (0, 0.25))
    assert set(t[:, 0].tolist()) == {0, 5, 6}
    g, b, s = (t[:, c].view(np.float32) for c in (1, 2, 3))
    assert g.min() >= 0.5 and g.max() <= 2.0 and b.min() >= -1 and b.max() <= 1 and s.min() >= 0 and s.max() <= 0.25
    assert len(np.unique(g)) > 500


# ---- the C ABI refuses bad arguments before it touches the device ------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from insar_unet_ca_amd import _lib
    return _lib.load()


FAKE = [0x10000 * (k + 1) for k in range(6)]         # never dereferenced: every call below is refused first


def _draw(lib, n=4, mask=0xff, gain=(1.0, 1.0), bias=(0.0, 0.0), sigma=(0.0, 0.0), table=FAKE[0]):
    return lib.insar_aug_draw(1, 2, n, mask, gain[0], gain[1], bias[0], bias[1], sigma[0], sigma[1], table, None)


def test_draw_argument_validation_without_a_gpu(lib):
    inf, nan = float("inf"), float("nan")
    assert _draw(lib, table=None) == E_ARG
    assert b"null" in lib.insar_last_error()
    for mask in (0, 256, -1, 1 << 20):
        assert _draw(lib, mask=mask) in (E_ARG, E_SHAPE)
        assert b"ops_mask" in lib.insar_last_error()
    for n in (0, -3):
        assert _draw(lib, n=n) in (E_ARG, E_SHAPE)
    for kw in ({"gain": (1.5, 1.0)}, {"bias": (0.1, -0.1)}, {"sigma": (0.2, 0.1)}, {"sigma": (-0.1, 0.1)},
               {"gain": (1.0, inf)}, {"gain": (nan, 1.0)}, {"bias": (-inf, 0.0)}, {"bias": (0.0, nan)}, {"sigma": (0.0, inf)},
               {"sigma": (nan, nan)}):
        assert _draw(lib, **kw) in (E_ARG, E_SHAPE), kw


def _apply(lib, x=FAKE[0], xo=FAKE[1], C=2, m=FAKE[2], md=2, mo=FAKE[3], n=2, H=8, W=8, table=FAKE[4]):
    return lib.insar_aug_apply(x, xo, C, m, md, mo, n, H, W, table, 7, None)


def test_apply_argument_validation_without_a_gpu(lib):
    from insar_unet_ca_amd import _lib
    assert (_lib.AUG_MASK_NONE, _lib.AUG_MASK_U8, _lib.AUG_MASK_I64) == (0, 1, 2)
    bad = (E_ARG, E_SHAPE)
    assert _apply(lib, xo=FAKE[0]) in bad and b"in-place" in lib.insar_last_error()          # x == xo
    assert _apply(lib, mo=FAKE[2]) in bad and b"in-place" in lib.insar_last_error()          # m == mo
    for kw in ({"n": 0}, {"C": 0}, {"H": 0}, {"W": 0}, {"n": -1}, {"H": 32769}, {"W": 32769}, {"H": 1 << 30}):
        assert _apply(lib, **kw) == E_SHAPE, kw
    for md in (3, -1, 64):
        assert _apply(lib, md=md) == E_DTYPE
    assert _apply(lib, xo=None) in bad and _apply(lib, x=None) in bad                       # a pointer without its partner
    assert _apply(lib, mo=None) in bad and _apply(lib, m=None) in bad
    assert _apply(lib, x=None, xo=None, m=None, mo=None, md=0) in bad                       # nothing to do
    assert _apply(lib, m=None, mo=None, md=2) in bad and _apply(lib, md=0) in bad           # pointers and dtype disagree
    assert _apply(lib, table=None) in bad and b"table" in lib.insar_last_error()
    # the binding raises on every one of them
    with pytest.raises(_lib.InsarError, match="in-place"):
        _lib.call("insar_aug_apply", FAKE[0], FAKE[0], 1, None, 0, None, 1, 8, 8, FAKE[4], 0, None)


# ---- Augment and the tta argument ------------------------------------------------------------------------------------------
def test_augment_argument_checks():
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import InsarError
    from insar_unet_ca_amd.augment import Augment
    assert iu.Augment is Augment and "Augment" in iu.__all__
    assert Augment().ops_mask == 0xff and Augment(ops="flips").ops_mask == 0x0f and Augment(ops=[0, 5, 6]).ops_mask == 0x61
    assert Augment(ops=iter([3])).ops_mask == 8
    for kw in ({"ops": "rot"}, {"ops": []}, {"ops": [8]}, {"ops": [-1]}, {"ops": [1.5]}, {"ops": 3}, {"gain": (2.0, 1.0)},
               {"bias": (0.0, float("inf"))}, {"noise_sigma": (-0.1, 0.1)}, {"noise_sigma": (0.3, 0.1)}, {"gain": 1.0},
               {"seed": -1}, {"rank": -2}, {"seed": 1.5}):
        with pytest.raises(InsarError):
            Augment(**kw)
    a = Augment(seed=3, rank=2)
    assert a.key_seed == ref.key_seed(3, 2) and a.noise_seed(9) == ref.noise_seed(3, 2, 9)
    assert Augment(seed=3, rank=1).key_seed != a.key_seed
    # host tensors are refused before anything is launched, and the step does not advance
    with pytest.raises(InsarError, match="ROCm"):
        a(torch.zeros(1, 1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64))
    assert a.step == 0


def test_state_dict_round_trip():
    from insar_unet_ca_amd import InsarError
    from insar_unet_ca_amd.augment import Augment
    a = Augment(seed=11, rank=3, ops=[0, 1, 6], gain=(0.8, 1.25), bias=(-0.1, 0.1), noise_sigma=(0.0, 0.05))
    a.step = 41
    sd = a.state_dict()
    assert set(sd) == {"seed", "rank", "step", "config"} and sd["seed"] == 11 and sd["rank"] == 3 and sd["step"] == 41
    b = Augment()
    b.load_state_dict(sd)
    assert b.state_dict() == sd and b.key_seed == a.key_seed and b.ops_mask == 0x43
    assert b.gain == a.gain and b.bias == a.bias and b.noise_sigma == a.noise_sigma and b.noise_seed(41) == a.noise_seed(41)
    import json
    c = Augment()
    c.load_state_dict(json.loads(json.dumps(sd)))                 # survives a JSON checkpoint
    assert c.state_dict() == sd
    for broken in ({}, {**sd, "config": {}}, {**sd, "step": -1}, {**sd, "config": {**sd["config"], "ops_mask": 0}}):
        with pytest.raises(InsarError):
            Augment().load_state_dict(broken)


@pytest.mark.parametrize("tta", [0, 3, 5, 6, 7, 16, -1, 2.0, "4", None, True])
def test_tta_values_other_than_1_2_4_8_are_refused(tta):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import InsarError
    net = torch.nn.Conv2d(1, 2, 1)
    with pytest.raises(InsarError, match="tta"):
        iu.ScenePredictor(net, tile=32, overlap=8, batch=2, tta=tta)
    with pytest.raises(InsarError, match="tta"):
        iu.predict_scene(net, np.zeros((64, 64), dtype=np.uint8), tile=32, overlap=8, tta=tta)
    with pytest.raises(InsarError, match="tta"):
        iu.detect_scene(net, np.zeros((64, 64), dtype=np.uint8), tile=32, overlap=8, tta=tta)


def test_tta_values_accepted():
    import insar_unet_ca_amd as iu
    net = torch.nn.Conv2d(1, 2, 1)
    assert iu.ScenePredictor(net, tile=32, overlap=8).tta == 1
    for tta in (1, 2, 4, 8):
        assert iu.ScenePredictor(net, tile=32, overlap=8, tta=tta).tta == tta


def test_transposing_op_on_a_non_square_shape_is_refused():
    """Augment raises before it draws or launches anything, and the step does not advance."""
    from insar_unet_ca_amd import InsarError
    from insar_unet_ca_amd.augment import Augment

    class FakeCuda(torch.Tensor):
        """A host tensor that claims to be a device tensor: lets Augment reach its shape rule, which precedes any launch."""
        @property
        def is_cuda(self):
            return True

    x = torch.zeros(2, 1, 8, 12).as_subclass(FakeCuda)
    a = Augment(ops="d4")
    with pytest.raises(InsarError, match="square"):
        a(x)
    assert a.step == 0
    with pytest.raises(InsarError, match="square"):
        Augment(ops=[0, 4])(x)
