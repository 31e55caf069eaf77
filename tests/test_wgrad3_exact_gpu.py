"""GPU: the four row-of-taps 3x3 weight-gradient kernels (csrc/wgrad3.hip, wgrad3x.hip, wgrad3y.hip, wgrad3k.hip) and the
first layer's three kernels (csrc/direct.hip: insar_conv3x3_small_fwd, _small_wgrad, _small_wgrad_fused) held ELEMENT-EXACTLY
to the integer references of tests/wgrad3_ref.py and tests/conv_ref.py (which tests/test_wgrad3_ref_host.py and
tests/test_conv_ref_host.py hold to torch.autograd in float64; the former also shows which planted staging / partition errors
the folded max_rel criterion of tests/test_parity_gpu.py lets through).

Operands are integers in {-1, 0, 1} over fewer than 2^24 pixels (asserted by the generator): every product is exact in bf16 /
fp32 and every partial sum, in ANY partition of the pixels, is an integer an fp32 accumulator holds exactly. So every route —
16x16x32 and 32x32x16 fragments, 64 / 128 / 256-wide tiles, the three LDS rings, pixel slices — has ONE right answer per slab,
and EVERY comparison in this file is torch.equal or its bitwise form. The reference is computed from the original integers on
the device with torch's float64 matmul, never with this project's kernels.

Every slab case (`_exact_slabs`), for nsplit in {1, 2, 3, ksteps // 2, ksteps, ksteps + 3} and one ragged value:
 - x and g are packed through engine.pack_input; `part` has one slab more than the launch may write, all NaN;
 - every slab in range equals wgrad3_ref.row_tap_slabs (splits without a K step: exact zeros), the guard slab is bitwise as
   filled, and the fold (ctx.wgrad_finish) equals conv3x3_weight_grad;
 - again with x as a channel slice (offset 64) of a wider buffer whose other channels hold 3 and dy as a slice (offset 64)
   of one whose other channels hold -7: the slabs are bitwise the plain run's;
 - the x probe and the dy probe (wgrad3_ref.probe_operands) at nsplit = 1 and the largest nsplit: a failure names the pixel
   the kernel fetched and the one it should have.
insar_wgrad_conv3x / 3y are also compared with insar_wgrad_conv3's slabs at the same nsplit (the documented bit-for-bit
claim), the 32x32x16 fragments (knob wgrad3_m32) with the same reference as the default ones. Nothing in this file skips."""
import pytest
import torch

from tests import conv_ref as R
from tests import wgrad3_ref as G

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SLICE_OFF, SLICE_EXTRA = 64, 128           # slice form: the slice's channel offset, channels beside it (64 before, 64 after)
X_FILL, DY_FILL = 3.0, -7.0                # what the channels beside the x / dy slices hold
NAN = float("nan")
_SWITCHES = ("WGRAD_ROWS", "WGRAD_X", "WGRAD_Y", "WGRAD_K", "WGRAD_K_TILES")
_AT_IMPORT = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib, engine
    _lib.load()                      # fail loudly if the extension is missing
    for k in _SWITCHES:
        v = getattr(engine, k)
        _AT_IMPORT.setdefault(k, set(v) if isinstance(v, set) else v)
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _untouched(t):
    return _same_bits(t, torch.full_like(t, NAN))


def _act(vals, dtype, dev, beside=None):
    """Integer NCHW values -> an Act through engine.pack_input, read back exactly; beside = fill: as the slice at SLICE_OFF
    of a buffer SLICE_EXTRA channels wider, whose other channels (halo included) hold `fill`."""
    from insar_unet_ca_amd import engine
    b, c, h, w = vals.shape
    if beside is None:
        a = engine.Act.alloc(b, h, w, c, dtype, dev)
    else:
        wide = engine.Act.alloc(b, h, w, c + SLICE_EXTRA, dtype, dev)
        wide.buf.fill_(beside)
        wide.buf[..., SLICE_OFF:SLICE_OFF + c] = 0
        a = wide.slice(SLICE_OFF, c)
    engine.pack_input(vals.float(), a)
    assert torch.equal(a.nchw().double(), vals.double()), "insar_pack_nchw"
    own = a.buf[..., a.c_off:a.c_off + a.c_len].float().clone()
    own[:, 1:-1, 1:-1] = 0
    assert not bool(own.any()), "halo of the slice"
    return a


def _raw(name, *args):
    """An entry point's return code, without _lib.call's exception."""
    from insar_unet_ca_amd import _lib
    return getattr(_lib.load(), name)(*args)


def _launch(entry, xa, ga, nsplit, slabs, guard=1):
    """part[slabs + guard][9][Co][Ci], NaN-prefilled, after one launch."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    part = torch.full((slabs + guard, 9, ga.c_len, xa.c_len), NAN, device=xa.buf.device)
    call(entry, xa.ref, ga.ref, ptr(part), nsplit, _lib.stream_ptr())
    torch.cuda.synchronize()
    return part


def _diff(got, want):
    bad = (got.double() != want.double())
    slabs = bad.flatten(1).any(1).nonzero().flatten().tolist()
    return f"{int(bad.sum())} of {want.numel()} elements differ, in slabs {slabs[:12]}"


def _nsplits(ksteps):
    ragged = next((n for n in range(4, ksteps) if ksteps % n), ksteps + 1)
    return sorted({1, 2, 3, max(1, ksteps // 2), ksteps, ksteps + 3, ragged})


_TILE = {"insar_wgrad_conv3": "insar_wgrad_conv3_tile", "insar_wgrad_conv3x": "insar_wgrad_conv3x_tile",
         "insar_wgrad_conv3y": "insar_wgrad_conv3y_tile", "insar_wgrad_conv3k": "insar_wgrad_conv3k_tile"}


def _exact_slabs(dev, entry, dtype, cin, cout, shape, tile, against=None, seed=31):
    """The steps of the module docstring for one (entry, layer, grid). tile: what the entry's _tile predicate must answer;
    against: another entry whose slabs must be bitwise these at every nsplit."""
    from insar_unet_ca_amd import engine
    from insar_unet_ca_amd._lib import call
    B, H, W = shape
    ctx = engine.Ctx(dev, dtype)
    o = G.integer_operands(seed, B, cin, cout, H, W, device=dev)
    xa, ga = _act(o.x, dtype, dev), _act(o.g, dtype, dev)
    xs, gs = _act(o.x, dtype, dev, X_FILL), _act(o.g, dtype, dev, DY_FILL)
    assert call(_TILE[entry], xa.ref, cout) == tile and call(_TILE[entry], xs.ref, cout) == tile
    slices = call("insar_wgrad_conv3k_slices", xa.ref, cout) if entry == "insar_wgrad_conv3k" else 1
    assert slices >= 1 and (entry != "insar_wgrad_conv3k" or slices == 8 // ((tile >> 16) // 64 * ((tile & 0xffff) // 64)))
    step = slices * G.SLICE if entry == "insar_wgrad_conv3k" else G.STEP
    ksteps = G.num_steps(B, H, W, step)
    what = f"{entry} {cin}->{cout} {shape} {'bf16' if dtype == BF16 else 'fp32'}"
    for nsplit in _nsplits(ksteps):
        tag = f"{what} nsplit {nsplit}"
        n = nsplit * slices
        want = G.row_tap_slabs(o.x, o.g, nsplit, step, slices)
        part = _launch(entry, xa, ga, nsplit, n)
        assert _untouched(part[n:]), tag + ": the slab behind the last one was written"
        assert not bool(torch.isnan(part[:n]).any()), tag + ": a slab in range was not fully written"
        assert torch.equal(part[:n].double(), want.double()), tag + ": " + _diff(part[:n], want)
        sps = -(-ksteps // nsplit)
        for s in range(nsplit):
            if s * sps >= ksteps:
                assert not bool(part[s * slices:(s + 1) * slices].any()), tag + f": split {s} has no K step and is not zero"
        gw = torch.full((cout, cin, 3, 3), NAN, device=dev)
        ctx.wgrad_finish(part[:n].reshape(-1), gw, n, 9, cout, cin, 0)
        torch.cuda.synchronize()
        assert torch.equal(gw.double(), o.dw.double()), tag + ": the folded gradient"
        sliced = _launch(entry, xs, gs, nsplit, n)
        assert _same_bits(sliced, part), tag + ": slice form is not bitwise the plain run"
        if against is not None:
            assert call(_TILE[against], xa.ref, cout)
            other = _launch(against, xa, ga, nsplit, n)
            assert torch.equal(other[:n], part[:n]), tag + f": not bitwise {against}'s slabs"
    assert bool((xs.buf[..., :SLICE_OFF] == X_FILL).all()) and bool((xs.buf[..., SLICE_OFF + cin:] == X_FILL).all())
    assert bool((gs.buf[..., :SLICE_OFF] == DY_FILL).all()) and bool((gs.buf[..., SLICE_OFF + cout:] == DY_FILL).all())
    for kind in ("x", "dy"):
        pr = G.probe_operands(kind, B, cin, cout, H, W, step, G.SLICE if slices > 1 else None, device=dev)
        pxa, pga = _act(pr.x, dtype, dev), _act(pr.g, dtype, dev)
        for nsplit in (1, ksteps + 3):
            n = nsplit * slices
            want = G.row_tap_slabs(pr.x, pr.g, nsplit, step, slices)
            part = _launch(entry, pxa, pga, nsplit, n)
            assert torch.equal(part[:n].double(), want.double()), \
                f"{what} nsplit {nsplit}: {G.probe_report(pr, part[:n]) or kind + ' probe: ' + _diff(part[:n], want)}"
            assert _untouched(part[n:])


def _id(cin, cout, shape):
    return f"{cin}x{cout}-" + "x".join(map(str, shape))


_GRIDS6 = [(2, 3, 64), (1, 2, 128), (2, 4, 32), (2, 8, 16), (3, 4, 16), (1, 1, 64)]
_GRIDS5 = [(2, 3, 64), (1, 2, 128), (2, 4, 32), (2, 8, 16), (1, 1, 64)]


@pytest.mark.parametrize("cin,cout,shape", [pytest.param(ci, co, s, id=_id(ci, co, s))
                                            for ci, co in ((64, 64), (128, 64), (64, 128), (128, 128)) for s in _GRIDS6])
def test_wgrad_conv3_bf16(dev, cin, cout, shape):
    """wgrad3_kernel<bf16_t, 64, 64, 4>, <128, 64, 4>, <64, 128, 4> and <128, 128, 8>. (3, 4, 16): one K step per image,
    every step with a top and a bottom halo row; (1, 1, 64): one K step in all."""
    tile = ((128 if cin % 128 == 0 else 64) << 16) | (128 if cout % 128 == 0 else 64)
    _exact_slabs(dev, "insar_wgrad_conv3", BF16, cin, cout, shape, tile)


@pytest.mark.parametrize("shape", _GRIDS6, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_conv3_bf16_32x32x16_fragments(dev, shape):
    """wgrad3_kernel<bf16_t, 128, 128, 8, 32> (knob wgrad3_m32 = 1: v_mfma_f32_32x32x16_bf16 fragments with their own LDS
    swizzle): the same reference, hence bit for bit the default fragments."""
    from insar_unet_ca_amd import _lib
    before = _lib.tune("wgrad3_m32")
    try:
        _lib.tune("wgrad3_m32", 1)
        assert _lib.tune("wgrad3_m32") == 1
        _exact_slabs(dev, "insar_wgrad_conv3", BF16, 128, 128, shape, (128 << 16) | 128)
    finally:
        _lib.tune("wgrad3_m32", before)


@pytest.mark.parametrize("cin,cout,shape", [pytest.param(c, c, s, id=_id(c, c, s)) for c in (64, 128)
                                            for s in ((2, 3, 64), (2, 4, 32), (2, 8, 16))])
def test_wgrad_conv3_fp32(dev, cin, cout, shape):
    """wgrad3_kernel<float, 64, 64, 4> and <float, 128, 128, 8> (v_mfma_f32_16x16x4_f32)."""
    _exact_slabs(dev, "insar_wgrad_conv3", F32, cin, cout, shape, (cin << 16) | cout)


@pytest.mark.parametrize("cin,cout,shape", [pytest.param(ci, co, s, id=_id(ci, co, s))
                                            for ci, co in ((256, 128), (128, 256)) for s in _GRIDS5])
def test_wgrad_conv3x(dev, cin, cout, shape):
    """wgrad3x_kernel<256, 128> and <128, 256>, W >= 64 (SINV) and W = 16 / 32; bit for bit insar_wgrad_conv3."""
    tile = (256 << 16) | 128 if cin == 256 else (128 << 16) | 256
    _exact_slabs(dev, "insar_wgrad_conv3x", BF16, cin, cout, shape, tile, against="insar_wgrad_conv3")


@pytest.mark.parametrize("cin,cout,shape", [pytest.param(ci, co, s, id=_id(ci, co, s))
                                            for ci, co in ((128, 128), (256, 128), (128, 384)) for s in _GRIDS5])
def test_wgrad_conv3y(dev, cin, cout, shape):
    """wgrad3y_kernel<128, 128>: one tile (the 128 -> 128 layers engine.WGRAD_Y & 2 sends here), two Cin tiles, three Cout
    tiles; bit for bit insar_wgrad_conv3."""
    _exact_slabs(dev, "insar_wgrad_conv3y", BF16, cin, cout, shape, (128 << 16) | 128, against="insar_wgrad_conv3")


_K_CASES = [(64, 64, 256), (128, 64, 128), (64, 128, 128), (128, 128, 64)]


@pytest.mark.parametrize("cin,cout,shape", [pytest.param(ci, co, s, id=_id(ci, co, s)) for ci, co, w in _K_CASES
                                            for s in ((2, 2, w), (1, 1, w), (1, 3, 2 * w))])
def test_wgrad_conv3k(dev, cin, cout, shape):
    """wgrad3k_kernel<64, 64> (KS = 8), <128, 64> and <64, 128> (KS = 4), <128, 128> (KS = 2): slab split * KS + slice holds
    the products of the split's pixels [slice * 32, slice * 32 + 32) of each K step — against the same reference as the
    other three kernels."""
    tile = ((128 if cin % 128 == 0 else 64) << 16) | (128 if cout % 128 == 0 else 64)
    _exact_slabs(dev, "insar_wgrad_conv3k", BF16, cin, cout, shape, tile)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
_REFUSED = [  # entry, dtype, cin, cout, (B, H, W), nsplit
    ("insar_wgrad_conv3", BF16, 64, 64, (1, 4, 48), 1), ("insar_wgrad_conv3", BF16, 64, 64, (2, 3, 32), 1),
    ("insar_wgrad_conv3", BF16, 96, 64, (1, 2, 64), 1), ("insar_wgrad_conv3", F32, 64, 96, (1, 2, 64), 1),
    ("insar_wgrad_conv3", BF16, 64, 64, (1, 2, 64), 0), ("insar_wgrad_conv3", F32, 128, 128, (1, 2, 64), -1),
    ("insar_wgrad_conv3x", BF16, 256, 128, (1, 4, 48), 1), ("insar_wgrad_conv3x", BF16, 256, 128, (2, 3, 32), 1),
    ("insar_wgrad_conv3x", BF16, 128, 128, (1, 2, 64), 1), ("insar_wgrad_conv3x", F32, 256, 128, (1, 2, 64), 1),
    ("insar_wgrad_conv3x", BF16, 256, 128, (1, 2, 64), 0),
    ("insar_wgrad_conv3y", BF16, 128, 128, (1, 4, 48), 1), ("insar_wgrad_conv3y", BF16, 128, 128, (2, 3, 32), 1),
    ("insar_wgrad_conv3y", BF16, 64, 128, (1, 2, 64), 1), ("insar_wgrad_conv3y", F32, 128, 128, (1, 2, 64), 1),
    ("insar_wgrad_conv3y", BF16, 128, 128, (1, 2, 64), 0),
    ("insar_wgrad_conv3k", BF16, 64, 64, (1, 2, 128), 1), ("insar_wgrad_conv3k", BF16, 128, 128, (1, 4, 48), 1),
    ("insar_wgrad_conv3k", BF16, 128, 128, (2, 2, 32), 1), ("insar_wgrad_conv3k", BF16, 96, 64, (1, 1, 256), 1),
    ("insar_wgrad_conv3k", F32, 128, 128, (1, 2, 64), 1), ("insar_wgrad_conv3k", BF16, 128, 128, (1, 2, 64), 0),
]


@pytest.mark.parametrize("entry,dtype,cin,cout,shape,nsplit", _REFUSED)
def test_refused_layers_write_nothing(dev, entry, dtype, cin, cout, shape, nsplit):
    """A layer the entry's _tile predicate rejects (W = 48; W = 32 with H = 3; 96 channels; fp32 for 3x / 3y / 3k; W = 128
    for wgrad3k's 64 x 64 tile; a tile the kernel does not have) and nsplit < 1: a nonzero return code, `part` untouched."""
    from insar_unet_ca_amd import _lib, engine
    from insar_unet_ca_amd._lib import ptr
    B, H, W = shape
    xa, ga = engine.Act.alloc(B, H, W, cin, dtype, dev), engine.Act.alloc(B, H, W, cout, dtype, dev)
    part = torch.full((max(nsplit, 1) * 8 + 1, 9, cout, cin), NAN, device=dev)
    if nsplit >= 1:
        assert _raw(_TILE[entry], xa.ref, cout) == 0
    else:
        assert _raw(_TILE[entry], xa.ref, cout) != 0
    assert _raw(entry, xa.ref, ga.ref, ptr(part), nsplit, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert _untouched(part)


# ---- the engine's dispatch -------------------------------------------------------------------------------------------------------
_ROUTES = [  # id, engine switches, entry for 128 -> 128 at (2, 4, 64), entry for 256 -> 128 at (2, 8, 16)
    ("default", {}, "insar_wgrad_conv3", "insar_wgrad_conv3x"),
    ("per-tap", {"WGRAD_ROWS": False}, "insar_wgrad", "insar_wgrad"),
    ("no-3x", {"WGRAD_X": False}, "insar_wgrad_conv3", "insar_wgrad_conv3"),
    ("3y-for-3x", {"WGRAD_Y": 1}, "insar_wgrad_conv3", "insar_wgrad_conv3y"),
    ("3y-for-128", {"WGRAD_Y": 2}, "insar_wgrad_conv3y", "insar_wgrad_conv3x"),
    ("3k", {"WGRAD_K": True, "WGRAD_K_TILES": {"64x64", "128x64", "64x128", "128x128"}}, "insar_wgrad_conv3k", "insar_wgrad_conv3x"),
]
_WGRAD_ENTRIES = {"insar_wgrad", "insar_wgrad_conv3", "insar_wgrad_conv3x", "insar_wgrad_conv3y", "insar_wgrad_conv3k"}


@pytest.mark.parametrize("switches,entry_a,entry_b", [pytest.param(s, a, b, id=i) for i, s, a, b in _ROUTES])
def test_engine_dispatch_is_exact_on_every_route(dev, monkeypatch, switches, entry_a, entry_b):
    """engine._wgrad_conv3 (its own split factor, its own fold) on the integer operands under each route; the entry that ran
    is the intended one."""
    from insar_unet_ca_amd import engine
    defaults = {"WGRAD_ROWS": True, "WGRAD_X": True, "WGRAD_Y": 0, "WGRAD_K": False}
    for k, v in {**defaults, **switches}.items():
        monkeypatch.setattr(engine, k, v)
    ctx = engine.Ctx(dev, BF16)
    for (cin, cout, shape), entry in (((128, 128, (2, 4, 64)), entry_a), ((256, 128, (2, 8, 16)), entry_b)):
        o = G.integer_operands(41, shape[0], cin, cout, shape[1], shape[2], device=dev)
        xa, ga = _act(o.x, BF16, dev), _act(o.g, BF16, dev)
        calls, orig = [], engine.call
        monkeypatch.setattr(engine, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
        gw = torch.full((cout, cin, 3, 3), NAN, device=dev)
        engine._wgrad_conv3(ctx, xa, ga, gw)
        torch.cuda.synchronize()
        monkeypatch.setattr(engine, "call", orig)
        assert [c for c in calls if c in _WGRAD_ENTRIES] == [entry], calls
        assert torch.equal(gw.double(), o.dw.double()), f"{entry} {cin}->{cout} {shape}: " + _diff(gw, o.dw)


# ---- the first layer ---------------------------------------------------------------------------------------------------------------
def _ints(gen, shape, lo=-1, hi=1):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cin", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(2, 5, 16), (1, 3, 40), (2, 2, 64)], ids=lambda s: "x".join(map(str, s)))
def test_first_layer_forward(dev, dtype, cin, shape):
    """insar_conv3x3_small_fwd (bf16 with Cin <= 3: the matrix-core kernel, the fp32 weight as a bf16 head plus remainder;
    otherwise the VALU kernel), dense integer x and w in {-1, 0, 1} (|y| <= 36): y equals conv_ref.conv3x3 with a zero halo;
    the NaN-prefilled statistics slab with two guard rows is fully written, sums to channel_stats(y) exactly and leaves the
    guard rows alone; again with y as a channel slice (offset 32) of a 128-channel buffer that holds -7 elsewhere."""
    from insar_unet_ca_amd import _lib, engine
    from insar_unet_ca_amd._lib import call, ptr
    B, H, W = shape
    gen = torch.Generator().manual_seed(100 + cin)
    x, w = _ints(gen, (B, cin, H, W)).to(dev), _ints(gen, (64, cin, 3, 3)).to(dev)
    want = R.conv3x3(x, w)
    R.assert_exact_in_bf16(want)
    R.assert_sums_exact_in_fp32(want)
    s1, s2 = R.channel_stats(want)
    wt = w.float().contiguous()
    xa = _act(x, dtype, dev)
    plain = None
    for sliced in (False, True):
        tag = f"small_fwd Cin {cin} {shape}" + (" (slice form)" if sliced else "")
        if sliced:
            wide = engine.Act.alloc(B, H, W, 128, dtype, dev)
            wide.buf.fill_(DY_FILL)
            wide.buf[..., 32:96] = 0
            ya = wide.slice(32, 64)
        else:
            ya = engine.Act.alloc(B, H, W, 64, dtype, dev)
        rows = call("insar_conv3x3_small_fwd_rows", xa.ref, ya.ref)
        assert 1 <= rows <= B * H
        stats = torch.full((rows + 2, 2, 64), NAN, device=dev)
        call("insar_conv3x3_small_fwd", xa.ref, ptr(wt), ya.ref, ptr(stats), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(ya.nchw().double(), want.double()), tag + ": " + _diff(ya.nchw(), want)
        own = ya.buf[..., ya.c_off:ya.c_off + 64].float().clone()
        own[:, 1:-1, 1:-1] = 0
        assert not bool(own.any()), tag + ": halo"
        assert _untouched(stats[rows:]), tag + ": statistics rows beyond the launch's were written"
        assert not bool(torch.isnan(stats[:rows]).any()), tag + ": a statistics row was not written"
        tot = stats[:rows].double().sum(0)
        assert torch.equal(tot[0], s1.double()) and torch.equal(tot[1], s2.double()), tag + ": statistics"
        if sliced:
            assert bool((wide.buf[..., :32] == DY_FILL).all()) and bool((wide.buf[..., 96:] == DY_FILL).all()), tag + ": beside y"
            assert _same_bits(ya.buf[..., 32:96], plain[0]) and _same_bits(stats, plain[1]), tag + ": not bitwise the plain run"
        else:
            plain = (ya.buf.clone(), stats)


def _small_wgrad(dev, dtype, x, g, what):
    """insar_conv3x3_small_wgrad on integer operands: the NaN-prefilled part[blocks + 1][Co*Ci*9] fully written, guard row
    untouched; returns the column sum through ctx.colsum as [64][Ci][3][3]."""
    from insar_unet_ca_amd import _lib, engine
    from insar_unet_ca_amd._lib import call, ptr
    B, cin, H, W = x.shape
    ctx = engine.Ctx(dev, dtype)
    xa, ga = _act(x, dtype, dev), _act(g, dtype, dev)
    nb, cols = call("insar_conv3x3_small_wgrad_blocks", B, H), 64 * cin * 9
    part = torch.full((nb + 1, cols), NAN, device=dev)
    call("insar_conv3x3_small_wgrad", xa.ref, ga.ref, ptr(part), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _untouched(part[nb:]), what + ": the row behind the last block's was written"
    assert not bool(torch.isnan(part[:nb]).any()), what + ": a block's row was not fully written"
    gw = torch.full((64, cin, 3, 3), NAN, device=dev)
    ctx.colsum(part, gw, 1, nb, cols)
    torch.cuda.synchronize()
    return gw


_SMALL_WGRAD = [(2, (2, 3, 64)), (2, (1, 5, 64)), (2, (3, 2, 192)), (2, (3, 4, 40)), (1, (2, 4, 64))]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cin,shape", _SMALL_WGRAD, ids=[f"cin{c}-" + "x".join(map(str, s)) for c, s in _SMALL_WGRAD])
def test_first_layer_weight_gradient(dev, dtype, cin, shape):
    """insar_conv3x3_small_wgrad: bf16 with Cin = 2 and W % 64 == 0 on the matrix cores ((1, 5, 64): fewer K steps than waves),
    (3, 4, 40) and Cin = 1 on the VALU kernel. Random integers against conv3x3_weight_grad, then the x probe: the bit code
    of the padded pixel index, Cin bits a launch, g one-hot at the hot pixels — a failure names the pixel fetched."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(200 + cin)
    x, g = _ints(gen, (B, cin, H, W)).to(dev), _ints(gen, (B, 64, H, W)).to(dev)
    what = f"small_wgrad Cin {cin} {shape}"
    gw = _small_wgrad(dev, dtype, x, g, what)
    want = G.conv3x3_weight_grad(x, g)
    assert torch.equal(gw.double(), want.double()), what + ": " + _diff(gw, want)
    pr = G.probe_operands("x", B, G.CODE_BITS, 64, H, W, 64, device=dev)          # hot pixels and g; x is rebuilt Cin bits at a time
    nbits = int(G.padded_index(B - 1, H - 1, W - 1, H, W)).bit_length()
    code = torch.zeros((1, 9, 64, G.CODE_BITS), device=dev)
    exact = True
    for first in range(0, nbits, cin):
        xb = G.code_image(B, H, W, cin, dev, first_bit=first, bits=cin)
        got = _small_wgrad(dev, dtype, xb, pr.g, what + " probe")
        exact = exact and torch.equal(got.double(), G.conv3x3_weight_grad(xb, pr.g).double())
        hi = min(first + cin, G.CODE_BITS)
        code[0, :, :, first:hi] = got.reshape(64, cin, 9).permute(2, 0, 1)[:, :, :hi - first]
    report = G.probe_report(pr, code)
    assert exact and report == "", what + ": " + (report or "probe launches differ from the reference")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", [(2, 3, 64), (1, 5, 64), (3, 2, 192)], ids=lambda s: "x".join(map(str, s)))
def test_first_layer_weight_gradient_with_the_apply_pass_inside(dev, shape, relu):
    """insar_conv3x3_small_wgrad_fused (bf16, Cin = 2, W % 64 == 0) against the header's formula in int64,
        dy = scale * (g * mask - k1 - (y - mean) * invstd * k2),   mask = relu ? [scale * y + shift > 0] : 1,
    followed by conv3x3_weight_grad: scale in {1, 2}, integer shift and mean, invstd = 1, k1 in {-1, 0, 1}, k2 in {0, 1},
    y in [-8, 8], g in {-1, 0, 1} — every dy an integer of magnitude <= 256. Some scale * y + shift are exactly 0: the mask is
    0 there (as insar_bnrelu_bwd_apply's), and the test would tell (the gradient under `>= 0` differs)."""
    from insar_unet_ca_amd import _lib, engine
    from insar_unet_ca_amd._lib import call, ptr
    B, H, W = shape
    gen = torch.Generator().manual_seed(300)
    x, g = _ints(gen, (B, 2, H, W)).to(dev), _ints(gen, (B, 64, H, W)).to(dev)
    y = _ints(gen, (B, 64, H, W), -8, 8).to(dev)
    scale, shift, mean = _ints(gen, (64,), 1, 2).to(dev), _ints(gen, (64,), -4, 4).to(dev), _ints(gen, (64,), -2, 2).to(dev)
    k1, k2 = _ints(gen, (64,)).to(dev), _ints(gen, (64,), 0, 1).to(dev)
    per_c = lambda v: v.reshape(1, 64, 1, 1)
    pre = per_c(scale) * y + per_c(shift)
    assert bool((pre == 0).any()) and bool((pre > 0).any()) and bool((pre < 0).any())

    def dy_of(mask):
        return per_c(scale) * (g * mask - per_c(k1) - (y - per_c(mean)) * per_c(k2))
    dy = dy_of((pre > 0).to(torch.int64) if relu else torch.ones_like(pre))
    R.assert_exact_in_bf16(dy)
    assert B * H * W * R.OUT_LIMIT < R.SUM_LIMIT
    want = G.conv3x3_weight_grad(x, dy)
    if relu:
        assert not torch.equal(G.conv3x3_weight_grad(x, dy_of((pre >= 0).to(torch.int64))), want)
    ctx = engine.Ctx(dev, BF16)
    xa, ga, ya = _act(x, BF16, dev), _act(g, BF16, dev), _act(y, BF16, dev)
    assert call("insar_conv3x3_small_wgrad_fused_ok", xa.ref, ya.ref) == 1
    vec = [v.float().contiguous() for v in (scale, shift, mean, torch.ones_like(scale), k1, k2)]
    nb, cols = call("insar_conv3x3_small_wgrad_blocks", B, H), 64 * 2 * 9
    part = torch.full((nb + 1, cols), NAN, device=dev)
    call("insar_conv3x3_small_wgrad_fused", xa.ref, ga.ref, ya.ref, *[ptr(v) for v in vec], relu, ptr(part), _lib.stream_ptr())
    torch.cuda.synchronize()
    what = f"small_wgrad_fused {shape} relu {relu}"
    assert _untouched(part[nb:]), what + ": the row behind the last block's was written"
    assert not bool(torch.isnan(part[:nb]).any()), what + ": a block's row was not fully written"
    gw = torch.full((64, 2, 3, 3), NAN, device=dev)
    ctx.colsum(part, gw, 1, nb, cols)
    torch.cuda.synchronize()
    assert torch.equal(gw.double(), want.double()), what + ": " + _diff(gw, want)


# ---- nothing leaks ---------------------------------------------------------------------------------------------------------------
def test_no_knob_and_no_engine_switch_leaks(dev):
    """Last in the file: the wgrad3_m32 knob reads 0 and the engine's WGRAD_* switches hold what they held before the first
    test of this file."""
    from insar_unet_ca_amd import _lib, engine
    assert _lib.tune("wgrad3_m32") == 0
    for k in _SWITCHES:
        assert getattr(engine, k) == _AT_IMPORT[k], k
