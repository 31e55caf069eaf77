"""GPU: insar_aug_draw / insar_aug_apply (csrc/augment.hip), Augment and DevicePrefetcher(augment=...) against the numpy
restatement in tests/augment_ref.py. Every comparison is bitwise: the kernels' arithmetic is fixed rounding for rounding
(floats are compared through their int32 view)."""
import numpy as np
import pytest
import torch

from tests import augment_ref as ref

pytestmark = pytest.mark.gpu
GUARD = 64               # elements of padding either side of a guarded output


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


def _same_i64(t: torch.Tensor, want: np.ndarray) -> bool:
    got = t.detach().cpu().numpy()
    return got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)


# ---- draw ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, step", [(0, 0), (0x123456789ABCDEF0, 7), ((1 << 64) - 1, (1 << 40) + 5)])
@pytest.mark.parametrize("ops_mask", [0xff, 0x0f, 0x61])
def test_draw_equals_the_oracle(dev, seed, step, ops_mask):
    from insar_unet_ca_amd import _lib
    n, gain, bias, sigma = 37, (0.75, 1.5), (-0.25, 0.125), (0.0, 0.3)
    table = torch.full((n + 2, 4), -7, dtype=torch.int32, device=dev)
    _lib.call("insar_aug_draw", seed, step, n, ops_mask, gain[0], gain[1], bias[0], bias[1], sigma[0], sigma[1],
              table[1:].data_ptr(), _lib.stream_ptr())
    got = table.cpu().numpy()
    assert np.array_equal(got[1:n + 1], ref.draw(seed, step, n, ops_mask, gain, bias, sigma))
    assert (got[0] == -7).all() and (got[n + 1] == -7).all()          # nothing outside the n rows


# ---- apply with explicit tables ------------------------------------------------------------------------------------------
N, C = 8, 2
GAINS = [1.25, 0.5, -1.5, 3.0, 0.875, 1.0625, 2.0, 0.3]
BIASES = [0.1, -0.2, 0.3, -0.4, 0.05, 1.5, -2.25, 0.7]
SIGMAS = [0.0, 0.25, 0.0, 1.0, 0.0625, 0.0, 0.5, 0.0]
NOISE_SEED = 0xC0FFEE1234567


def _inputs(H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    m64 = rng.choice(np.array([0, 1, 2, 255, -100, (1 << 40) + 3], dtype=np.int64), size=(N, H, W))
    m8 = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    return x, m64, m8


def _guarded(numel, dtype, dev, fill):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def _run_apply(dev, x, m, table, x_offset=0):
    """apply on the device with outputs inside guarded buffers -> (xo, mo) tensors; asserts that the guards are untouched."""
    from insar_unet_ca_amd.augment import apply_table
    xd = md = xo = mo = xbuf = mbuf = None
    if x is not None:
        if x_offset:                                   # the input starts `x_offset` floats past a 16-byte boundary
            holder = torch.zeros(x.size + 4, dtype=torch.float32, device=dev)
            assert holder.data_ptr() % 16 == 0
            xd = holder[x_offset:x_offset + x.size].view(x.shape)
            xd.copy_(torch.from_numpy(x))
            assert xd.data_ptr() % 16 == 4 * x_offset
        else:
            xd = torch.from_numpy(x).to(dev)
        xbuf, xo = _guarded(x.size, torch.float32, dev, -777.0)
        xo = xo.view(x.shape)
    if m is not None:
        md = torch.from_numpy(m).to(dev)
        mbuf, mo = _guarded(m.size, torch.int64, dev, -777)
        mo = mo.view(m.shape)
    rx, rm = apply_table(xd, md, torch.from_numpy(table).to(dev), NOISE_SEED, out=(xo, mo))
    assert (rx is None) == (x is None) and (rm is None) == (m is None)
    torch.cuda.synchronize()
    for buf in (xbuf, mbuf):
        if buf is not None:
            assert bool((buf[:GUARD] == -777).all()) and bool((buf[-GUARD:] == -777).all()), "wrote outside the output"
    return rx, rm


SHAPES = [(72, 72), (70, 70), (1, 1), (64, 64), (48, 80)]


@pytest.mark.parametrize("H, W", SHAPES)
@pytest.mark.parametrize("mask_kind", ["int64", "uint8"])
def test_apply_all_ops_in_one_batch(dev, H, W, mask_kind):
    x, m64, m8 = _inputs(H, W, seed=H * 1000 + W)
    m = m64 if mask_kind == "int64" else m8
    table = ref.make_table(list(range(8)), GAINS, BIASES, SIGMAS)
    xo, mo = _run_apply(dev, x, m, table)
    want_x, want_m = ref.apply(x, m, table, NOISE_SEED)
    assert _same_f32(xo, want_x)
    assert _same_i64(mo, want_m)
    if mask_kind == "int64":
        assert {-100, (1 << 40) + 3, 255} <= set(np.unique(want_m).tolist()) or H * W == 1


def test_apply_with_x_off_the_16_byte_boundary(dev):
    x, m64, _ = _inputs(72, 72, seed=5)
    table = ref.make_table(list(range(8)), GAINS, BIASES, SIGMAS)
    xo, mo = _run_apply(dev, x, m64, table, x_offset=1)
    want_x, want_m = ref.apply(x, m64, table, NOISE_SEED)
    assert _same_f32(xo, want_x) and _same_i64(mo, want_m)


@pytest.mark.parametrize("H, W", [(72, 72), (48, 80), (70, 70)])
def test_apply_with_garbage_op_words(dev, H, W):
    """Only op & 7 counts (and bit 2 is dropped on a non-square plane): no table content leads outside the planes."""
    x, m64, _ = _inputs(H, W, seed=9)
    ops = [0x7fffffff, -1, -2147483648, 0x12345678, 8, -8, 0x7ffffff5, 1 << 20 | 6]
    table = ref.make_table(ops, GAINS, BIASES, SIGMAS)
    xo, mo = _run_apply(dev, x, m64, table)
    clean = table.copy()
    clean[:, 0] &= 7
    want_x, want_m = ref.apply(x, m64, clean, NOISE_SEED)
    assert _same_f32(xo, want_x) and _same_i64(mo, want_m)


@pytest.mark.parametrize("H, W", [(72, 72), (70, 70)])
def test_apply_image_only_and_mask_only(dev, H, W):
    x, m64, m8 = _inputs(H, W, seed=13)
    table = ref.make_table([7, 6, 5, 4, 3, 2, 1, 0], GAINS, BIASES, SIGMAS)
    want_x, want_m = ref.apply(x, m64, table, NOISE_SEED)
    xo, none = _run_apply(dev, x, None, table)
    assert none is None and _same_f32(xo, want_x)
    none, mo = _run_apply(dev, None, m64, table)
    assert none is None and _same_i64(mo, want_m)
    none, mo = _run_apply(dev, None, m8, table)
    assert _same_i64(mo, ref.apply(None, m8, table)[1])


def test_apply_refuses_what_the_kernel_cannot_do(dev):
    from insar_unet_ca_amd import InsarError
    from insar_unet_ca_amd.augment import apply_table
    x = torch.zeros(2, 1, 8, 8, device=dev)
    t = torch.from_numpy(ref.make_table([0, 1], [1, 1], [0, 0], [0, 0])).to(dev)
    with pytest.raises(InsarError, match="in-place"):
        apply_table(x, None, t, out=(x, None))
    with pytest.raises(InsarError, match="table"):
        apply_table(x, None, t[:1])
    with pytest.raises(InsarError, match="masks"):
        apply_table(x, torch.zeros(2, 8, 8, dtype=torch.int32, device=dev), t)
    with pytest.raises(InsarError, match="float32"):
        apply_table(x.double(), None, t)


# ---- Augment -------------------------------------------------------------------------------------------------------------
AUG_KW = dict(ops="d4", gain=(0.8, 1.25), bias=(-0.1, 0.1), noise_sigma=(0.0, 0.2))


def _oracle_call(x, m, seed, rank, step, ops_mask=0xff, kw=AUG_KW):
    table = ref.draw(ref.key_seed(seed, rank), step, x.shape[0], ops_mask, kw["gain"], kw["bias"], kw["noise_sigma"])
    return ref.apply(x, m, table, ref.noise_seed(seed, rank, step))


def test_augment_streams(dev):
    from insar_unet_ca_amd import Augment
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, 2, 40, 40)).astype(np.float32)
    m = rng.integers(0, 3, size=(5, 40, 40)).astype(np.int64)
    xd, md = torch.from_numpy(x).to(dev), torch.from_numpy(m).to(dev)
    a, b = Augment(seed=7, rank=1, **AUG_KW), Augment(seed=7, rank=1, **AUG_KW)
    a.step = b.step = 3
    ax, am = a(xd, md)
    bx, bm = b(xd, md)
    assert a.step == 4 and ax.data_ptr() != xd.data_ptr() and am.dtype == torch.int64
    want_x, want_m = _oracle_call(x, m, 7, 1, 3)
    assert _same_f32(ax, want_x) and _same_i64(am, want_m)
    assert torch.equal(ax.view(torch.int32), bx.view(torch.int32)) and torch.equal(am, bm)
    # the next step, another rank and another seed all differ
    nx, _ = a(xd, md)
    assert not torch.equal(nx, ax) and _same_f32(nx, _oracle_call(x, m, 7, 1, 4)[0])
    for other in (Augment(seed=7, rank=2, **AUG_KW), Augment(seed=8, rank=1, **AUG_KW)):
        other.step = 3
        assert not torch.equal(other(xd, md)[0], ax)
    # a resumed object continues the stream
    c = Augment()
    c.load_state_dict(b.state_dict())
    assert c.step == 4 and _same_f32(c(xd, md)[0], _oracle_call(x, m, 7, 1, 4)[0])
    # a side stream gives what the default stream gives
    side = torch.cuda.Stream(device=dev)
    d = Augment(seed=7, rank=1, **AUG_KW)
    d.step = 3
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        sx, sm = d(xd, md)
    side.synchronize()
    assert torch.equal(sx.view(torch.int32), ax.view(torch.int32)) and torch.equal(sm, am)
    # uint8 masks come back int64
    ux, um = Augment(seed=1, ops="flips")(xd, md.to(torch.uint8))
    assert um.dtype == torch.int64 and _same_i64(um, _oracle_call(x, m, 1, 0, 0, 0x0f, dict(gain=(1, 1), bias=(0, 0), noise_sigma=(0, 0)))[1])


def test_augment_refuses_a_transposing_op_on_non_square_tiles(dev):
    from insar_unet_ca_amd import Augment, InsarError
    x = torch.zeros(2, 1, 16, 24, device=dev)
    a = Augment(ops="d4")
    with pytest.raises(InsarError, match="square"):
        a(x)
    assert a.step == 0
    out, none = Augment(ops="flips")(x)
    assert none is None and out.shape == x.shape


# ---- DevicePrefetcher ------------------------------------------------------------------------------------------------------
def _loader(values):
    rng = np.random.default_rng(17)
    batches = []
    for k in range(5):
        n = 4 if k < 4 else 3
        x = rng.standard_normal((n, 2, 32, 32)).astype(np.float32)
        m = rng.choice(np.asarray(values, dtype=np.int64), size=(n, 32, 32))
        batches.append((torch.from_numpy(x), torch.from_numpy(m)))
    return batches


@pytest.mark.parametrize("path, values, compact", [("compact", [0, 1, 255], True), ("plain", [0, 1, 255], False),
                                                   ("plain-by-value", [0, 1, -100], True)])
def test_prefetcher_with_augment(dev, path, values, compact):
    from insar_unet_ca_amd import Augment, DevicePrefetcher
    batches = _loader(values)
    aug = Augment(seed=21, rank=0, **AUG_KW)
    pf = DevicePrefetcher(batches, dev, compact_masks=compact, augment=aug)
    seen = 0
    for k, (xb, mb) in enumerate(pf):
        assert xb.is_cuda and xb.dtype == torch.float32 and mb.dtype == torch.int64
        want_x, want_m = _oracle_call(batches[k][0].numpy(), batches[k][1].numpy(), 21, 0, k)
        assert _same_f32(xb, want_x), f"{path}: images of batch {k}"
        assert _same_i64(mb, want_m), f"{path}: masks of batch {k}"
        seen += 1
    assert seen == 5 and aug.step == 5
    if path == "compact":
        assert pf._dev_u8[0] is not None          # the uint8 buffer was the kernel's source
    # a second pass continues the stream
    xb, mb = next(iter(pf))
    assert _same_f32(xb, _oracle_call(batches[0][0].numpy(), batches[0][1].numpy(), 21, 0, 5)[0])


@pytest.mark.parametrize("compact", [True, False])
def test_prefetcher_without_augment_yields_the_loaders_tensors(dev, compact):
    from insar_unet_ca_amd import DevicePrefetcher
    batches = _loader([0, 1, 255])
    pf = DevicePrefetcher(batches, dev, compact_masks=compact)
    assert pf.augment is None
    n = 0
    for (xb, mb), (x, m) in zip(pf, batches):
        assert torch.equal(xb.cpu().view(torch.int32), x.view(torch.int32)) and mb.dtype == torch.int64 and torch.equal(mb.cpu(), m)
        n += 1
    assert n == 5 and all(a is None for a in pf._aug)
