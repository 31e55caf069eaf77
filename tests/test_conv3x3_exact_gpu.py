"""GPU: the 3x3 forward / input-gradient kernels held ELEMENT-EXACTLY to tests/conv_ref.py's integer reference (which
tests/test_conv_ref_host.py holds to torch.nn.functional in float64 and to autograd; that file also shows which planted
indexing errors the float64 tolerances of tests/test_parity_gpu.py let through):

 * the 64 -> 64 rolling-window kernel (csrc/conv3x3_c64.hip);
 * the 8-wave flat kernel (csrc/conv3x3_flat.hip): plain, ping-pong, persistent, row tiles, dilated row tiles;
 * the two-work-group kernel (csrc/conv3x3_flat2.hip), flat geometry and row tiles, one tile per group and persistent;
 * the per-tap implicit GEMM (csrc/igemm.hip, mode 0) with its epilogue options (bias, add, gate, strided output).

Operands are small integers (conv_ref.integer_operands: x, g in {-1, 0, 1}, sparse w in {-1, 0, 1}) for which every output
is an integer of magnitude <= 256 and every per-channel sum stays below 2^24 — asserted by the generator — so fp32
accumulation in any order, the bf16 store and the fp32 statistics are all exact: there is one right answer, and EVERY
comparison in this file is torch.equal (or its bitwise form). The reference is computed from the original integer tensors
(on the device, with torch's float64 matmul; never with this project's kernels), not from anything read back, so the same
assertions cover insar_pack_nchw, insar_unpack_nchw and insar_weight_prep*.

Every case (`_exact`): pack x and g, build the GemmWeight, forward with a statistics slab, input gradient; then
 - y and dx equal the reference, through Act.nchw() and through insar_unpack_nchw; the halo is zero;
 - the slab starts as NaN with two rows more than the launch's row count: rows [0, rows) are all written and sum to
   (sum y, sum y^2) exactly, the rows beyond stay bitwise as filled;
 - the whole case again with x / g as a channel slice (offset 64) of a wider buffer whose other channels hold 3, and y / dx
   as a slice (offset 32) of a wider buffer whose other channels hold -7: those come back unchanged and the slice is bitwise
   the plain run, as is the slab.
Variants documented as bit for bit equal are compared with torch.equal: ping-pong / persistent against the plain loop, row
tiles against the flat geometry, the dilated row tiles against the per-tap kernel's out-of-bounds variant; and — with integer
operands the fp32 summation order cannot matter — the two-work-group kernel against the 8-wave kernel.

Skips. Only the carried-sum cases can skip, when the device has so many compute units that the persistent launch runs one
work-group per tile and nothing is carried: test_flat_8wave[carried-*] (as tests/test_conv_epilogue_gpu.py does). The
32 -> 64 two-work-group case has no input gradient (its output would have 32 columns; the kernels need multiples of 64):
that half is not launched, nothing is skipped."""
import ctypes as C

import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
IN_OFF, OUT_OFF, EXTRA = 64, 32, 64        # slice form: channel offsets of the input / output slices, channels beside them
IN_FILL, OUT_FILL = 3.0, -7.0              # what the channels beside the slices hold


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()                      # fail loudly if the extension is missing
    return torch.device("cuda:0")


# ---- operands: one reference per (layer, shape), shared by the cases that follow one another -------------------------------
_OPS = {}


def _ops(dev, cin, cout, shape, dil=1, stride=1):
    key = (cin, cout, tuple(shape), dil, stride)
    if key not in _OPS:
        while len(_OPS) >= 2:
            _OPS.pop(next(iter(_OPS)))
        B, H, W = shape
        _OPS[key] = R.integer_operands(2024 + dil, B, cin, cout, H, W, dil, stride, device=dev)
    return _OPS[key]


def _desc(shape, c, dtype):
    """A descriptor for the host-side geometry queries (they do not touch the buffer)."""
    from insar_unet_ca_amd import _lib
    B, H, W = shape
    return C.byref(_lib.InsarAct(0x1000, B, H, W, c, 0, c, _lib.dtype_code(dtype), 0))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _act(vals, dtype, dev, layout=None):
    """Integer NCHW values -> an Act through engine.pack_input (insar_pack_nchw), read back exactly. layout "in" / "out": as
    the slice of a wider buffer that the slice form uses for inputs / outputs."""
    from insar_unet_ca_amd import engine
    b, c, h, w = vals.shape
    a = _alloc(b, h, w, c, dtype, dev, layout)[0]
    engine.pack_input(vals.float(), a)
    assert torch.equal(a.nchw().double(), vals.double()), "insar_pack_nchw"
    assert _halo_is_zero(a)
    return a


def _alloc(b, h, w, c, dtype, dev, layout=None):
    """(Act, wide buffer's Act or None)."""
    from insar_unet_ca_amd import engine
    if layout is None:
        return engine.Act.alloc(b, h, w, c, dtype, dev), None
    off, fill = (IN_OFF, IN_FILL) if layout == "in" else (OUT_OFF, OUT_FILL)
    wide = engine.Act.alloc(b, h, w, c + EXTRA, dtype, dev)
    wide.buf.fill_(fill)
    wide.buf[..., off:off + c] = 0
    return wide.slice(off, c), wide


def _beside_unchanged(a, wide, fill):
    lo, hi = wide.buf[..., :a.c_off], wide.buf[..., a.c_off + a.c_len:]
    return bool((lo == fill).all()) and bool((hi == fill).all())


def _own(a):
    return a.buf[..., a.c_off:a.c_off + a.c_len]


def _halo_is_zero(a):
    t = _own(a).float().clone()
    t[:, 1:-1, 1:-1] = 0
    return not bool(t.any())


def _weights(dev, dtype, o):
    """The GemmWeight of o.w, its two GEMM-operand forms (insar_weight_prep) checked against the original integers."""
    from insar_unet_ca_amd import engine
    ctx = engine.Ctx(dev, dtype)
    cout, cin = o.w.shape[:2]
    gw = engine.GemmWeight(ctx, torch.nn.Parameter(o.w.float().contiguous()), "conv3")
    assert torch.equal(gw.fwd().double(), o.w.permute(2, 3, 0, 1).reshape(9, cout, cin).double()), "insar_weight_prep (fwd)"
    assert torch.equal(gw.dgrad().double(), o.w.permute(2, 3, 1, 0).reshape(9, cin, cout).double()), "insar_weight_prep (dgrad)"
    return gw


def _equal_ints(got, want, what):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, what
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} elements differ"


def _check_slab(slab, rows, want_y, what):
    nan_rows = torch.full_like(slab[rows:], float("nan"))
    assert _same_bits(slab[rows:], nan_rows), f"{what}: rows beyond the {rows} the launch writes were touched"
    body = slab[:rows].double()
    assert not bool(torch.isnan(body).any()), f"{what}: a slab row below {rows} was not written"
    R.assert_sums_exact_in_fp32(want_y)
    s1, s2 = R.channel_stats(want_y)
    tot = body.sum(0)
    assert torch.equal(tot[0], s1.double()), f"{what}: sum y, {int((tot[0] != s1.double()).sum())} channels differ"
    assert torch.equal(tot[1], s2.double()), f"{what}: sum y^2, {int((tot[1] != s2.double()).sum())} channels differ"


def _exact(dev, dtype, o, fwd, bwd, rows, want_y=None, want_dx=None, stats_of=None, what=""):
    """The steps of the module docstring. fwd(xa, ya, wf, slab, aux) and bwd(ga, dxa, wd, aux) launch; aux(vals) makes an
    Act with the output's layout (for `add` / `gate`); rows: slab rows the forward launch writes, None = no slab;
    bwd None: no input gradient; stats_of: what the slab sums where that is not the stored y. Returns the plain run's
    (y Act, dx Act, slab)."""
    from insar_unet_ca_amd import engine
    want_y = o.y if want_y is None else want_y
    want_dx = o.dx if want_dx is None else want_dx
    R.assert_exact_in_bf16(want_y, want_dx)
    gw = _weights(dev, dtype, o)
    cout, cin = o.w.shape[:2]
    plain = None
    for sliced in (False, True):
        tag = what + (" (slice form)" if sliced else "")
        lin, lout = ("in", "out") if sliced else (None, None)
        aux = lambda vals: _act(vals, dtype, dev, lout)
        xa = _act(o.x, dtype, dev, lin)
        b, _, ho, wo = want_y.shape
        ya, ywide = _alloc(b, ho, wo, cout, dtype, dev, lout)
        slab = None if rows is None else torch.full((rows + 2, 2, cout), float("nan"), device=dev)
        fwd(xa, ya, gw.fwd(), slab, aux)
        dxa = dwide = None
        if bwd is not None:
            ga = _act(o.g, dtype, dev, lin)
            dxa, dwide = _alloc(b, o.x.shape[2], o.x.shape[3], cin, dtype, dev, lout)
            bwd(ga, dxa, gw.dgrad(), aux)
        torch.cuda.synchronize()
        if not sliced:
            _equal_ints(ya.nchw(), want_y, tag + " y")
            _equal_ints(engine.unpack_output(ya), want_y, tag + " y through insar_unpack_nchw")
            assert _halo_is_zero(ya), tag + " y halo"
            if dxa is not None:
                _equal_ints(dxa.nchw(), want_dx, tag + " dx")
                assert _halo_is_zero(dxa), tag + " dx halo"
            if slab is not None:
                _check_slab(slab, rows, want_y if stats_of is None else stats_of, tag)
            plain = (ya, dxa, slab)
        else:
            assert _same_bits(_own(ya), plain[0].buf), tag + " y is not bitwise the plain run"
            assert _beside_unchanged(ya, ywide, OUT_FILL), tag + " channels beside y were written"
            _equal_ints(engine.unpack_output(ya), want_y, tag + " y through insar_unpack_nchw")
            if dxa is not None:
                assert _same_bits(_own(dxa), plain[1].buf), tag + " dx is not bitwise the plain run"
                assert _beside_unchanged(dxa, dwide, OUT_FILL), tag + " channels beside dx were written"
            if slab is not None:
                assert _same_bits(slab, plain[2]), tag + " slab is not bitwise the plain run"
    return plain


def _flat(flags):
    """fwd / bwd launches of insar_conv3x3_flat with these flip bits."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr

    def fwd(xa, ya, wf, slab, aux=None):
        call("insar_conv3x3_flat", xa.ref, ya.ref, ptr(wf), flags, ptr(slab), _lib.stream_ptr())

    def bwd(ga, dxa, wd, aux=None):
        call("insar_conv3x3_flat", ga.ref, dxa.ref, ptr(wd), flags | 1, 0, _lib.stream_ptr())
    return fwd, bwd


def _equals_variant(dev, dtype, o, plain, flags, what):
    """The plain run's y and dx, bit for bit, from insar_conv3x3_flat with other flip bits (no slab)."""
    gw = _weights(dev, dtype, o)
    fwd, bwd = _flat(flags)
    xa = _act(o.x, dtype, dev)
    ya = _alloc(plain[0].B, plain[0].H, plain[0].W, plain[0].c_len, dtype, dev)[0]
    fwd(xa, ya, gw.fwd(), None)
    assert torch.equal(ya.buf, plain[0].buf), f"{what}: y differs from flip {flags}"
    if plain[1] is not None:
        ga = _act(o.g, dtype, dev)
        dxa = _alloc(plain[1].B, plain[1].H, plain[1].W, plain[1].c_len, dtype, dev)[0]
        bwd(ga, dxa, gw.dgrad())
        assert torch.equal(dxa.buf, plain[1].buf), f"{what}: dx differs from flip {flags | 1}"


# ---- layout conversion and weight re-layout on their own ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_pack_and_unpack_are_exact(dev, dtype):
    """insar_pack_nchw / insar_unpack_nchw on odd extents, every integer bf16 holds (|v| <= 256), plain and as slices."""
    from insar_unet_ca_amd import engine
    vals = torch.randint(-256, 257, (3, 24, 5, 7), generator=torch.Generator().manual_seed(1), dtype=torch.int64).to(dev)
    for layout, fill in ((None, None), ("in", IN_FILL), ("out", OUT_FILL)):
        a, wide = _alloc(3, 5, 7, 24, dtype, dev, layout)
        engine.pack_input(vals.float(), a)
        torch.cuda.synchronize()
        _equal_ints(_own(a)[:, 1:-1, 1:-1].permute(0, 3, 1, 2), vals, "insar_pack_nchw")
        _equal_ints(engine.unpack_output(a), vals, "insar_unpack_nchw")
        assert _halo_is_zero(a)
        assert wide is None or _beside_unchanged(a, wide, fill)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_batched_weight_relayout_of_integer_weights(dev, dtype):
    """insar_weight_prep and the one-launch paired form (engine.WeightSet.refresh) against permutations of the ORIGINAL
    integers (tests/test_parity_gpu.py compares with the device's own cast of the master)."""
    from insar_unet_ca_amd import engine
    ctx = engine.Ctx(dev, dtype)
    shapes = [("conv3", (128, 64, 3, 3)), ("conv3", (64, 192, 3, 3)), ("convT", (128, 64, 2, 2)), ("conv3", (33, 7, 3, 3)),
              ("conv3", (256, 128, 1, 1))]
    gen = torch.Generator().manual_seed(9)
    ints = [torch.randint(-256, 257, shp, generator=gen, dtype=torch.int64) for _, shp in shapes]
    params = [torch.nn.Parameter(v.float().to(dev)) for v in ints]
    single = [engine.GemmWeight(ctx, p, kind) for p, (kind, _) in zip(params, shapes)]
    batched = [engine.GemmWeight(ctx, p, kind) for p, (kind, _) in zip(params, shapes)]
    engine.WeightSet(ctx, batched).refresh()
    torch.cuda.synchronize()
    for (kind, shp), v, a, b in zip(shapes, ints, single, batched):
        v = v.to(dev)
        T = shp[2] * shp[3]
        if kind == "conv3":     # (Co,Ci,k,k) -> [tap][co][ci] and [tap][ci][co]
            fwd, dgr = v.permute(2, 3, 0, 1).reshape(T, shp[0], shp[1]), v.permute(2, 3, 1, 0).reshape(T, shp[1], shp[0])
        else:                   # (Ci,Co,2,2) -> [tap][co][ci] and [tap][ci][co]
            fwd, dgr = v.permute(2, 3, 1, 0).reshape(4, shp[1], shp[0]), v.permute(2, 3, 0, 1).reshape(4, shp[0], shp[1])
        for got in (a.fwd(), b._buf["fwd"]):
            _equal_ints(got, fwd, f"{kind} {shp} fwd")
        for got in (a.dgrad(), b._buf["dgrad"]):
            _equal_ints(got, dgr, f"{kind} {shp} dgrad")


# ---- the 64 -> 64 rolling-window kernel ---------------------------------------------------------------------------------------
def _c64_ring_batch():
    """The smallest batch of 256 x 256 images with more tiles than work-groups (a work-group walks several tiles, the ring wraps)."""
    from insar_unet_ca_amd._lib import call
    out = (C.c_int32 * 6)()
    for B in range(1, 9):
        d = _desc((B, 256, 256), 64, BF16)
        assert call("insar_conv3x3_c64_geometry", d, C.addressof(out)) == 1
        if out[4] > call("insar_conv3x3_c64_rows", d):
            return B
    raise AssertionError("no batch up to 8 gives the 64 -> 64 kernel more tiles than work-groups")


@pytest.mark.parametrize("shape", [(3, 30, 30), (1, 33, 300), (1, 16, 16), "ring"],
                         ids=["straddle-3x30x30", "long-rows-1x33x300", "tiny-1x16x16", "ring-wraps-256x256"])
def test_c64(dev, shape):
    """insar_conv3x3_c64, flip 0 and 1: tiles that straddle images, rows longer than a tile, fewer pixels than two tiles,
    and several tiles per work-group. One slab row per work-group, every one written."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    if shape == "ring":
        shape = (_c64_ring_batch(), 256, 256)
    d = _desc(shape, 64, BF16)
    assert call("insar_conv3x3_c64_ok", d, 64) == 1
    rows = call("insar_conv3x3_c64_rows", d)
    o = _ops(dev, 64, 64, shape)

    def fwd(xa, ya, wf, slab, aux):
        call("insar_conv3x3_c64", xa.ref, ya.ref, ptr(wf), 0, ptr(slab), _lib.stream_ptr())

    def bwd(ga, dxa, wd, aux):
        call("insar_conv3x3_c64", ga.ref, dxa.ref, ptr(wd), 1, 0, _lib.stream_ptr())
    _exact(dev, BF16, o, fwd, bwd, rows, what=f"c64 {shape}")


# ---- the 8-wave flat kernel -----------------------------------------------------------------------------------------------------
_FLAT_SHAPES = [(64, 128, (2, 40, 56)), (128, 64, (1, 33, 300)), (64, 64, (3, 30, 30)), (256, 128, (1, 32, 32))]
_FLAT_CASES = [pytest.param(cin, cout, shp, dt, fl, False, id=f"{cin}-{cout}-{'x'.join(map(str, shp))}-{'f32' if dt == F32 else 'bf16'}-flip{fl}")
               for cin, cout, shp in _FLAT_SHAPES for dt, fl in ((F32, 0), (BF16, 0), (BF16, 2), (BF16, 4), (BF16, 6))]
_FLAT_CASES += [pytest.param(64, cout, (1, 256, 256), BF16, fl, True, id=f"carried-64-{cout}-1x256x256-bf16-flip{fl}")
                for cout in (128, 64) for fl in (4, 6)]


@pytest.mark.parametrize("cin,cout,shape,dtype,flags,carried", _FLAT_CASES)
def test_flat_8wave(dev, cin, cout, shape, dtype, flags, carried):
    """insar_conv3x3_flat without bit 5: the plain loop (fp32 and bf16), ping-pong steps (2), persistent work-groups (4) and
    both (6); the latter three bit for bit the plain loop. carried: 263 tiles, one more step than a 256-group persistent
    grid, so the sums are carried over tile boundaries and folded once per work-group."""
    from insar_unet_ca_amd._lib import call
    d = _desc(shape, cin, dtype)
    mtiles = call("insar_conv3x3_flat_num_mtiles", d)
    rows = call("insar_conv3x3_flat_stat_rows", d, cout, flags)
    assert rows <= mtiles and (flags & 4 or rows == mtiles)
    if carried:
        assert mtiles == 263
        if not rows < mtiles:
            pytest.skip("this device runs the launch with one work-group per tile: nothing is carried")
    o = _ops(dev, cin, cout, shape)
    plain = _exact(dev, dtype, o, *_flat(flags), rows, what=f"flat flip {flags}")
    if flags:
        _equals_variant(dev, dtype, o, plain, 0, f"flat flip {flags}")


def _rows_h(W):
    return 2 * (256 // W)          # the smallest multiple of 256 / W with two tiles per image


_ROW_CASES = [(cin, cout, (2, _rows_h(W), W), fl) for (cin, cout, W) in ((64, 64, 16), (64, 128, 32), (128, 128, 64), (128, 64, 128), (64, 128, 256))
              for fl in (8 | 2, 8 | 2 | 16)]
_ROW_CASES += [(64, 256, (1, 64, 64), 8 | 2),        # N = 256: two N tiles of 128
               (128, 256, (2, 16, 16), 8 | 2 | 16)]   # narrow: 64-column tiles although N is a multiple of 128


@pytest.mark.parametrize("cin,cout,shape,flags", _ROW_CASES)
def test_flat_8wave_row_tiles(dev, cin, cout, shape, flags):
    """Row tiles (flip 8 | 2, with 16: 64-column tiles), one shape per W in {16 .. 256}, each with two tiles per image and two
    images (the N = 256 and the narrow case have their own shapes); bit for bit the flat geometry."""
    from insar_unet_ca_amd._lib import call
    d = _desc(shape, cin, BF16)
    assert call("insar_conv3x3_flat_rows_ok", d, cout) == 1 and call("insar_conv3x3_flat_rows_ok", _desc(shape, cout, BF16), cin) == 1
    rows = call("insar_conv3x3_flat_stat_rows", d, cout, flags)
    assert rows == shape[0] * shape[1] * shape[2] // 256
    o = _ops(dev, cin, cout, shape)
    plain = _exact(dev, BF16, o, *_flat(flags), rows, what=f"row tiles flip {flags}")
    _equals_variant(dev, BF16, o, plain, 2, "row tiles against the flat geometry")


@pytest.mark.parametrize("cin,cout,shape,dil,narrow", [
    (64, 128, (2, 32, 32), 2, False), (128, 64, (2, 32, 32), 4, True), (64, 64, (1, 16, 64), 2, False), (64, 128, (3, 8, 32), 3, False)])
def test_flat_8wave_dilated_row_tiles(dev, cin, cout, shape, dil, narrow):
    """Dilated row tiles (flip bits 8-11) and, on the same operands, the per-tap kernel's out-of-bounds variant: both equal
    the reference, hence each other."""
    from insar_unet_ca_amd import engine
    from insar_unet_ca_amd._lib import call
    d = _desc(shape, cin, BF16)
    assert call("insar_conv3x3_flat_rows_dil_ok", d, cout, dil) == 1 and call("insar_conv3x3_flat_rows_dil_ok", _desc(shape, cout, BF16), cin, dil) == 1
    flags = 8 | 2 | (16 if narrow else 0) | (dil << 8)
    rows = call("insar_conv3x3_flat_stat_rows", d, cout, flags)
    assert rows == shape[0] * shape[1] * shape[2] // 256
    o = _ops(dev, cin, cout, shape, dil)
    plain = _exact(dev, BF16, o, *_flat(flags), rows, what=f"dilation {dil}")
    taps = [(ky * dil - dil, kx * dil - dil) for ky in range(3) for kx in range(3)]
    _, h, w = shape

    def fwd(xa, ya, wf, slab, aux):
        engine._igemm(xa, ya, wf, cout, h, w, 1, taps, 0, stats=slab, oob=True)

    def bwd(ga, dxa, wd, aux):
        engine._igemm(ga, dxa, wd, cin, h, w, 1, [(-a, -b) for a, b in taps], 0, oob=True)
    oob = _exact(dev, BF16, o, fwd, bwd, call("insar_igemm_num_mtiles", shape[0] * h * w, cout), what=f"per-tap oob, dilation {dil}")
    assert torch.equal(plain[0].buf, oob[0].buf) and torch.equal(plain[1].buf, oob[1].buf)


# ---- the two-work-group kernel ------------------------------------------------------------------------------------------------
_FLAT2_SHAPES = [(32, 64, (3, 30, 30)),        # one slab: the loop is its tail only; tiles straddle images; no input gradient
                 (64, 128, (2, 40, 56)), (128, 64, (1, 33, 300)),
                 (64, 64, (3, 16, 16)), (128, 128, (3, 8, 64)), (128, 64, (2, 3, 256)),       # row tiles: W = 16, 64, 256
                 (64, 64, (10, 128, 128))]      # 640 row tiles: persistent with uneven shares
_FLAT2_CASES = [(cin, cout, shp, fl) for cin, cout, shp in _FLAT2_SHAPES
                for fl in ((32, 32 | 4) + ((32 | 8, 32 | 8 | 4) if shp[2] in (16, 64, 128, 256) else ()))]


@pytest.mark.parametrize("cin,cout,shape,flags", _FLAT2_CASES)
def test_flat_two_work_groups(dev, cin, cout, shape, flags):
    """insar_conv3x3_flat with bit 5, one tile per work-group and persistent (4), flat geometry and row tiles (8). Its
    documented difference from the 8-wave kernel is the fp32 summation order, which integers do not feel: bit for bit."""
    from insar_unet_ca_amd._lib import call
    d = _desc(shape, cin, BF16)
    rows_ok = call("insar_conv3x3_flat2_rows_ok", d, cout)
    assert rows_ok == (1 if shape[2] in (16, 64, 128, 256) and shape[1] % (256 // shape[2]) == 0 else 0)
    assert rows_ok or not flags & 8
    rows = call("insar_conv3x3_flat_stat_rows", d, cout, flags)
    mtiles = shape[0] * shape[1] * shape[2] // 256 if flags & 8 else call("insar_conv3x3_flat_num_mtiles", d)
    assert rows <= mtiles and (flags & 4 or rows == mtiles)
    o = _ops(dev, cin, cout, shape)
    fwd, bwd = _flat(flags)
    plain = _exact(dev, BF16, o, fwd, bwd if cin % 64 == 0 else None, rows, what=f"flat2 flip {flags}")
    if cin % 64 == 0:
        _equals_variant(dev, BF16, o, plain, 0, f"flat2 flip {flags} against the 8-wave kernel")


# ---- the per-tap implicit GEMM ------------------------------------------------------------------------------------------------
def _igemm_launches(cin, cout, shape, fwd_kw=None, bwd_kw=None):
    from insar_unet_ca_amd import engine
    _, h, w = shape

    def fwd(xa, ya, wf, slab, aux):
        kw = fwd_kw(aux) if fwd_kw else {}
        engine._igemm(xa, ya, wf, cout, h, w, 1, engine._TAPS3, 0, stats=slab, **kw)

    def bwd(ga, dxa, wd, aux):
        kw = bwd_kw(aux) if bwd_kw else {}
        engine._igemm(ga, dxa, wd, cin, h, w, 1, engine._TAPS3_DGRAD, 0, **kw)
    return fwd, bwd


@pytest.mark.parametrize("cin,cout,shape,dtype,tile_rows,tile_cols", [
    (64, 64, (3, 4, 4), F32, 128, 64), (64, 64, (3, 4, 4), BF16, 128, 64),                 # 48 pixels: M smaller than one tile
    (128, 64, (1, 8, 24), F32, 128, 64), (128, 64, (1, 8, 24), BF16, 128, 64),             # 192 pixels: a partial M tile
    (64, 64, (3, 120, 200), F32, 256, 64), (64, 64, (3, 120, 200), BF16, 256, 64),         # 256-row tiles, ragged last tile
    (64, 128, (4, 128, 128), BF16, 256, 128),                                              # 128-column tiles
    (64, 512, (2, 128, 128), BF16, 256, 256),                                              # 256 x 256 tiles (ping-pong K loop)
])
def test_igemm(dev, cin, cout, shape, dtype, tile_rows, tile_cols):
    """engine._igemm mode 0, forward with statistics and input gradient; the tile variant asserted through the library's
    own selectors (the input gradient of the last two has N = 64: 64-column tiles)."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    M = shape[0] * shape[1] * shape[2]
    assert call("insar_igemm_tile_rows", M, cout) == tile_rows
    assert call("insar_igemm_tile_cols_dt", M, cout, _lib.dtype_code(dtype)) == tile_cols
    o = _ops(dev, cin, cout, shape)
    _exact(dev, dtype, o, *_igemm_launches(cin, cout, shape), call("insar_igemm_num_mtiles", M, cout), what="igemm")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("option", ["bias", "add", "gate", "bias+add+gate"])
@pytest.mark.parametrize("cin,cout,shape", [(128, 64, (1, 8, 24)), (64, 128, (3, 37, 41))])
def test_igemm_epilogue_options(dev, cin, cout, shape, option, dtype):
    """bias (integers in [-5, 5]), add ({-1, 0, 1}, a tensor with the output's layout), gate (the stored result is zero
    where an integer gate tensor with zeros, negatives and positives is <= 0), forward and input gradient. Statistics where
    the interface takes them (without gate): the slab holds the sums of the GEMM result BEFORE bias and add — the "raw
    (bias-free) conv output" that insar_bn_finalize asks for — so it is held to the statistics of the plain convolution."""
    from insar_unet_ca_amd._lib import call
    o = _ops(dev, cin, cout, shape)
    gen = torch.Generator().manual_seed(77)

    def ints(lo, hi, *shp):
        return torch.randint(lo, hi + 1, shp, generator=gen, dtype=torch.int64).to(dev)
    want, extra = {}, {}
    for key, base, n in (("y", o.y, cout), ("dx", o.dx, cin)):
        v = base
        bias = ints(-5, 5, n) if "bias" in option else None
        add = ints(-1, 1, *base.shape) if "add" in option else None
        gate = ints(-2, 2, *base.shape) if "gate" in option else None
        if bias is not None:
            v = v + bias.reshape(1, n, 1, 1)
        if add is not None:
            v = v + add
        if gate is not None:
            assert bool((gate == 0).any()) and bool((gate < 0).any()) and bool((gate > 0).any())
            v = torch.where(gate <= 0, torch.zeros_like(v), v)
        want[key], extra[key] = v, (bias, add, gate)
    R.assert_exact_in_bf16(want["y"], want["dx"])            # the bound re-checked after bias / add

    def kw(key):
        bias, add, gate = extra[key]
        return lambda aux: dict(bias=None if bias is None else bias.float(), add=None if add is None else aux(add),
                                gate=None if gate is None else aux(gate))
    rows = None if "gate" in option else call("insar_igemm_num_mtiles", shape[0] * shape[1] * shape[2], cout)
    _exact(dev, dtype, o, *_igemm_launches(cin, cout, shape, kw("y"), kw("dx")), rows, want["y"], want["dx"], stats_of=o.y,
           what=f"igemm {option}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cin,cout,shape", [(64, 128, (2, 9, 12)), (128, 64, (3, 16, 7))])
def test_igemm_stride_2_and_its_input_gradient_by_parity_classes(dev, cin, cout, shape, dtype):
    """A stride-2 3x3 convolution (padding 1) forward, and its input gradient issued the way deeplab.ConvUnit does: one
    launch per parity class (py, px) of the input pixel with out_stride=2, out_off=(py, px), the class's taps selected
    from the [tap][ci][co] operand. Every interior pixel is written by exactly one class; the halo stays zero."""
    from insar_unet_ca_amd import engine
    from insar_unet_ca_amd._lib import call
    B, H, W = shape
    o = _ops(dev, cin, cout, shape, 1, 2)
    Ho, Wo = o.y.shape[2:]
    assert (Ho, Wo) == (R.out_size(H, 2), R.out_size(W, 2))

    def fwd(xa, ya, wf, slab, aux):
        engine._igemm(xa, ya, wf, cout, Ho, Wo, 2, engine._TAPS3, 0, stats=slab)

    def bwd(ga, dxa, wd, aux):
        for py in (0, 1):
            for px in (0, 1):
                sel = [(i, t) for i, t in enumerate(engine._TAPS3) if (t[0] - py) % 2 == 0 and (t[1] - px) % 2 == 0]
                hc, wc = (H - py + 1) // 2, (W - px + 1) // 2
                assert sel and hc > 0 and wc > 0
                buf = torch.index_select(wd, 0, torch.tensor([i for i, _ in sel], dtype=torch.int64, device=dev)).contiguous()
                taps = [((py - t[0]) // 2, (px - t[1]) // 2) for _, t in sel]
                engine._igemm(ga, dxa, buf, cin, hc, wc, 1, taps, 0, out_stride=2, out_off=(py, px))
    _exact(dev, dtype, o, fwd, bwd, call("insar_igemm_num_mtiles", B * Ho * Wo, cout), what="igemm stride 2")
