"""The generic weight-gradient path at the C ABI, launch by launch, against tests/wgrad_ref.py (which
tests/test_wgrad_ref_host.py holds to torch.autograd): insar_pixel_table / insar_pixel_table_taps, insar_wgrad (every
kernel instantiation its launcher can pick, slab by slab before any fold), insar_wgrad_fold / insar_wgrad_reduce (directly
and through Ctx.wgrad_finish at its 48- and 96-split thresholds), insar_colsum_ld / insar_colsum_partial.

Exact arithmetic instead of a tolerance: operands are small integers (|v| <= 3: exact in bf16 and fp32), so every product
and every fp32 partial sum is an integer far below 2^24 and each slab element has ONE right answer whatever the summation
order: torch.equal against the int64 reference. A pixel dropped, read twice, or taken from the wrong tap or channel cannot
pass. The slab buffers are prefilled with NaN, so an unwritten element shows. One random-valued case per dtype covers
non-trivial mantissas, at the tolerance test_igemm_family_against_float64 uses for weight gradients (KERNEL_TOL * 5)."""
import ctypes as C

import pytest
import torch

from oracle import closed_form as cf
from tests import wgrad_ref as R
from tests.helpers import max_rel
from tests.test_parity_gpu import KERNEL_TOL      # weight gradients there are held to KERNEL_TOL * 5

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()                      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _ints(seed, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def _act_of(vals, dtype, dev, c_off=0, c_len=None):
    """A padded NHWC buffer whose interior holds the NCHW tensor `vals` (every channel of the buffer, so that a read from a
    neighbouring channel is not a read of zeros) and whose halo is zero; returned as the slice [c_off, c_off + c_len)."""
    from insar_unet_ca_amd import engine
    b, c, h, w = vals.shape
    a = engine.Act.alloc(b, h, w, c, dtype, dev)
    a.buf[:, 1:-1, 1:-1] = vals.permute(0, 2, 3, 1).to(dev).to(dtype)
    return a if c_len is None else a.slice(c_off, c_len)


def _table(dev, B, H, W, s, Hb, Wb, tail):
    """insar_pixel_table, read back and held to the reference before anything is addressed through it."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    mpad = R.round_up(B * H * W, 64)
    t = torch.full((mpad,), -1, dtype=torch.int32, device=dev)
    call("insar_pixel_table", ptr(t), mpad, B, H, W, s, Hb, Wb, tail, _lib.stream_ptr())
    torch.cuda.synchronize()
    ref = R.pixel_table(B, H, W, s, Hb, Wb, tail, mpad)
    assert torch.equal(t.cpu().long(), ref), ("insar_pixel_table", B, H, W, s, Hb, Wb, tail)
    return t, ref


def _taps_table(dev, B, H, W, s, Hb, Wb, taps):
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    mpad = R.round_up(B * H * W, 64)
    t = torch.full((len(taps) * mpad,), -1, dtype=torch.int32, device=dev)
    dy = (C.c_int8 * 12)(*([a for a, _ in taps] + [0] * (12 - len(taps))))
    dx = (C.c_int8 * 12)(*([b for _, b in taps] + [0] * (12 - len(taps))))
    call("insar_pixel_table_taps", ptr(t), mpad, B, H, W, s, Hb, Wb, len(taps), C.addressof(dy), C.addressof(dx), _lib.stream_ptr())
    torch.cuda.synchronize()
    ref = R.pixel_table_taps(B, H, W, s, Hb, Wb, taps, mpad)
    assert torch.equal(t.cpu().long().view(len(taps), mpad), ref), ("insar_pixel_table_taps", B, H, W, s, Hb, Wb, taps)
    return t, ref


def _wgrad(dev, x, dy, tabx, tabdy, offx, offdy, nsplit, tap_stride=0):
    """One insar_wgrad launch into NaN-prefilled slabs: part[nsplit][ntaps][Cout][Cin]."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import InsarWgrad, call, ptr
    ntaps, cin, cout = len(offx), x.c_len, dy.c_len
    part = torch.full((nsplit, ntaps, cout, cin), NAN, device=dev)
    d = InsarWgrad()
    d.x, d.dy = x.desc, dy.desc
    d.tabx, d.tabdy, d.part = ptr(tabx), ptr(tabdy), ptr(part)
    d.Mpad, d.nsplit, d.ntaps = tabdy.numel(), nsplit, ntaps
    for i in range(ntaps):
        d.offx[i], d.offdy[i] = int(offx[i]), int(offdy[i])
    d.tabx_tap_stride = tap_stride
    call("insar_wgrad", C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    return part


def _check_slabs(got, ref, what):
    assert not bool(torch.isnan(got).any()), (what, "slab elements left unwritten")
    ref32 = ref.to(torch.float32)
    assert float(ref.abs().max()) < 2 ** 24
    g = got.cpu()
    if not torch.equal(g, ref32):
        bad = (g != ref32).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} slab elements differ, first at [split, tap, co, ci] = "
                             f"{bad[0].tolist()}: {float(g[tuple(bad[0])])} vs {float(ref32[tuple(bad[0])])}")


# ---- tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (1, 8, 8), (3, 5, 7), (2, 16, 24)])       # 128, 64, 105 (-> Mpad 128), 768 pixels
@pytest.mark.parametrize("s", [1, 2])
def test_pixel_table(dev, B, H, W, s):
    for tail in (0, W * s + 3):
        _table(dev, B, H, W, s, H * s, W * s, tail)


@pytest.mark.parametrize("B", [2, 1])
@pytest.mark.parametrize("s,taps", [
    (1, [(d * (r - 1), d * (c - 1)) for r in range(3) for c in range(3)]) for d in (1, 2, 12)] + [
    (2, [(0, 0)]),                                                                       # 1x1 stride 2 (a downsample conv)
    (2, [(r - 1, c - 1) for r in range(3) for c in range(3)]),                           # 3x3 stride 2
])
def test_pixel_table_taps(dev, B, s, taps):
    """8 x 8 maps: at dilation 12 every off-centre tap is out of bounds, at 2 a two-pixel rim of each is."""
    _taps_table(dev, B, 8 // s, 8 // s, s, 8, 8, taps)
    if s == 1:
        _taps_table(dev, 3, 5, 7, 1, 5, 7, taps)          # 105 pixels: entries beyond the grid are 0


# ---- insar_wgrad: every instantiation, slab by slab -------------------------------------------------------------------------
_INSTANCES = [      # dtype, Cin, Cout, expected (Cin tile, Cout tile)
    (BF16, 256, 256, (256, 256)),      # 8 waves
    (BF16, 128, 128, (128, 128)),
    (BF16, 256, 128, (128, 128)),
    (BF16, 128, 64, (128, 64)),
    (BF16, 64, 128, (64, 128)),
    (BF16, 64, 64, (64, 64)),
    (F32, 128, 128, (128, 128)),       # 8 waves
    (F32, 64, 64, (64, 64)),
    (F32, 128, 64, (64, 64)),
]
_GRIDS = [      # (B, h, w), split factors
    ((2, 8, 8), [1, 2]),                       # 128 pixels: 2 K steps
    ((1, 8, 8), [1]),                          # 1 K step
    ((3, 5, 7), [1, 2]),                       # 105 pixels: tail entries live (x reads the zero halo, dy a non-zero pixel)
    ((2, 16, 24), [1, 2, 3, 5, 12, 15]),       # 12 K steps: one, several, ragged steps per split, splits with no step
]


def _convT_arrangement(dev, dtype, cin, cout, grid, seed, x_extra=0, dy_concat=False):
    """UpPlan's weight-gradient operands: x (B, h, w, Cin), dy (B, 2h, 2w, Cout), tabx at stride 1 and tabdy at stride 2
    with tail 0, offdy = a*(2w+2) + b. x_extra: x is the slice at c_off = x_extra of a wider buffer; dy_concat: dy is the
    upper half (c_off = Cout) of a 2*Cout buffer."""
    B, h, w = grid
    xv = _ints(seed, -3, 3, B, cin + x_extra, h, w)
    gv = _ints(seed + 1, -3, 3, B, cout * (2 if dy_concat else 1), 2 * h, 2 * w)
    xa = _act_of(xv, dtype, dev, x_extra, cin)
    ga = _act_of(gv, dtype, dev, cout if dy_concat else 0, cout)
    tabx, rx = _table(dev, B, h, w, 1, h, w, 0)
    tabdy, rdy = _table(dev, B, h, w, 2, 2 * h, 2 * w, 0)
    offdy = [a * (2 * w + 2) + b for a, b in R.TAPS2]
    xr = R.pad_nhwc(xv[:, x_extra:x_extra + cin])
    gr = R.pad_nhwc(gv[:, cout:] if dy_concat else gv)
    return xa, ga, tabx, tabdy, offdy, (xr, gr, rx, rdy)


@pytest.mark.parametrize("grid,splits", _GRIDS)
@pytest.mark.parametrize("dtype,cin,cout,tile", _INSTANCES)
def test_wgrad_transposed_conv_slabs_are_exact(dev, dtype, cin, cout, tile, grid, splits):
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    assert call("insar_wgrad_tile_pair", cin, cout, _lib.dtype_code(dtype)) == (tile[0] << 16) | tile[1]
    xa, ga, tabx, tabdy, offdy, (xr, gr, rx, rdy) = _convT_arrangement(dev, dtype, cin, cout, grid, 100 + cin + cout)
    for nsplit in splits:
        ref = R.wgrad_slabs(xr, gr, rx, rdy, [0] * 4, offdy, nsplit)          # also asserts every address in bounds
        got = _wgrad(dev, xa, ga, tabx, tabdy, [0] * 4, offdy, nsplit)
        _check_slabs(got, ref, (str(dtype), cin, cout, grid, nsplit))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_wgrad_on_channel_slices_as_the_up_path_calls_it(dev, dtype):
    """x = channels [64, 64 + Cin) of a wider buffer, dy = the upper half of a 2*Cout concat buffer (UpPlan.backward)."""
    cin, cout, grid = 128, 64, (3, 5, 7)
    xa, ga, tabx, tabdy, offdy, (xr, gr, rx, rdy) = _convT_arrangement(dev, dtype, cin, cout, grid, 7, x_extra=64, dy_concat=True)
    assert (xa.c_off, xa.C, ga.c_off, ga.C) == (64, cin + 64, cout, 2 * cout)
    for nsplit in (1, 2):
        ref = R.wgrad_slabs(xr, gr, rx, rdy, [0] * 4, offdy, nsplit)
        _check_slabs(_wgrad(dev, xa, ga, tabx, tabdy, [0] * 4, offdy, nsplit), ref, (str(dtype), "slices", nsplit))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_wgrad_3x3_arrangement_slabs_are_exact(dev, dtype):
    """9 taps moving on x through offx (negative offsets included), x tail = the first interior pixel."""
    B, H, W, cin, cout = 3, 5, 7, 64, 64
    xv, gv = _ints(21, -3, 3, B, cin, H, W), _ints(22, -3, 3, B, cout, H, W)
    xa, ga = _act_of(xv, dtype, dev), _act_of(gv, dtype, dev)
    tabx, rx = _table(dev, B, H, W, 1, H, W, W + 3)
    tabdy, rdy = _table(dev, B, H, W, 1, H, W, 0)
    offx = [(r - 1) * (W + 2) + (c - 1) for r in range(3) for c in range(3)]
    assert min(offx) < 0
    for nsplit in (1, 2, 3):
        ref = R.wgrad_slabs(R.pad_nhwc(xv), R.pad_nhwc(gv), rx, rdy, offx, [0] * 9, nsplit)
        _check_slabs(_wgrad(dev, xa, ga, tabx, tabdy, offx, [0] * 9, nsplit), ref, (str(dtype), "3x3", nsplit))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_wgrad_per_tap_tables_slabs_are_exact(dev, dtype):
    """tabx_tap_stride != 0: a 3x3 conv at dilation 2 on 8 x 8 maps, out-of-bounds taps reading pixel 0."""
    B, H, W, cin, cout = 2, 8, 8, 64, 64
    taps = [(2 * (r - 1), 2 * (c - 1)) for r in range(3) for c in range(3)]
    xv, gv = _ints(31, -3, 3, B, cin, H, W), _ints(32, -3, 3, B, cout, H, W)
    xa, ga = _act_of(xv, dtype, dev), _act_of(gv, dtype, dev)
    tabx, rx = _taps_table(dev, B, H, W, 1, H, W, taps)
    tabdy, rdy = _table(dev, B, H, W, 1, H, W, 0)
    mpad = rdy.numel()
    assert int((rx == 0).sum()) > 0
    for nsplit in (1, 2):
        ref = R.wgrad_slabs(R.pad_nhwc(xv), R.pad_nhwc(gv), rx.reshape(-1), rdy, [0] * 9, [0] * 9, nsplit, tabx_tap_stride=mpad)
        _check_slabs(_wgrad(dev, xa, ga, tabx, tabdy, [0] * 9, [0] * 9, nsplit, tap_stride=mpad), ref, (str(dtype), "taps", nsplit))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_wgrad_random_values_against_float64(dev, dtype):
    """Non-trivial mantissas: the folded gradient against float64 on the kernel's own operands."""
    from insar_unet_ca_amd import _lib, engine
    from insar_unet_ca_amd._lib import call, ptr
    B, h, w, cin, cout = 2, 8, 8, 128, 64
    xa = engine.Act.alloc(B, h, w, cin, dtype, dev)
    engine.pack_input(cf.make_input((B, cin, h, w)).to(dev), xa)
    ga = engine.Act.alloc(B, 2 * h, 2 * w, cout, dtype, dev)
    engine.pack_input(cf.make_grad((B, cout, 2 * h, 2 * w)).to(dev), ga)
    tabx, rx = _table(dev, B, h, w, 1, h, w, 0)
    tabdy, rdy = _table(dev, B, h, w, 2, 2 * h, 2 * w, 0)
    offdy = [a * (2 * w + 2) + b for a, b in R.TAPS2]
    part = _wgrad(dev, xa, ga, tabx, tabdy, [0] * 4, offdy, 2)
    grad = torch.full((cin, cout, 4), NAN, device=dev)
    call("insar_wgrad_reduce", ptr(part), ptr(grad), 2, 4, cout, cin, 1, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    ref = R.reduce(R.wgrad_slabs(R.pad_nhwc(xa.nchw().cpu().double()), R.pad_nhwc(ga.nchw().cpu().double()), rx, rdy,
                                 [0] * 4, offdy, 2), 1)
    assert max_rel(grad, ref) <= KERNEL_TOL * 5


# ---- fold and reduce on synthetic slabs -------------------------------------------------------------------------------------
_SHAPES = [(64, 64, 0), (64, 192, 0), (3, 6, 0), (64, 128, 1)]     # (Co, Ci, float offset of `part`): a ragged 128-wide ci tile,
#                                                                   the scalar branch (Ci % 4), unaligned slabs (scalar branch)
_JUNK = 12345.0       # what lies behind the caller's last slab: a fold or reduce that reads past nsplit cannot sum to the reference
_MAX_FLOATS = 4 << 20  # 16 MB of slabs per case


def _slabs(dev, seed, nsplit, ntaps, co, ci, off):
    """Integer slabs (|v| <= 1000: any order of summation is exact in fp32) inside an allocation that runs 16 slabs past
    nsplit, filled with _JUNK there."""
    slab = ntaps * co * ci
    ref = _ints(seed, -1000, 1000, nsplit, ntaps, co, ci)
    store = torch.full((off + (nsplit + 16) * slab,), _JUNK, device=dev)
    part = store[off:off + nsplit * slab]
    part.copy_(ref.reshape(-1).to(torch.float32))
    return store, part, ref


@pytest.mark.parametrize("co,ci,off", _SHAPES)
@pytest.mark.parametrize("layout", [0, 1])
def test_wgrad_reduce_is_exact(dev, co, ci, off, layout):
    """insar_wgrad_reduce alone: the 8-deep tree of the 16-byte branch (4-deep of the scalar branch) and its remainder,
    both layouts, 1 to 12 taps, overwrite and accumulate."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    shape = (co, ci) if layout == 0 else (ci, co)
    for nsplit in (1, 3, 4, 7, 8, 9, 15, 16, 17, 47, 48):
        for ntaps in (1, 4, 9, 12):
            if nsplit * ntaps * co * ci > _MAX_FLOATS:
                continue
            store, part, ref = _slabs(dev, nsplit * 13 + ntaps, nsplit, ntaps, co, ci, off)
            assert (part.data_ptr() % 16 == 0) == (off == 0)
            before = store.clone()
            want = R.reduce(ref, layout)
            grad = torch.full(shape + (ntaps,), NAN, device=dev)
            call("insar_wgrad_reduce", ptr(part), ptr(grad), nsplit, ntaps, co, ci, layout, 0, _lib.stream_ptr())
            torch.cuda.synchronize()
            assert torch.equal(grad.cpu(), want.to(torch.float32)), ("overwrite", nsplit, ntaps)
            base = _ints(nsplit + ntaps, -500, 500, *shape, ntaps)
            grad = base.to(torch.float32).to(dev)
            call("insar_wgrad_reduce", ptr(part), ptr(grad), nsplit, ntaps, co, ci, layout, 1, _lib.stream_ptr())
            torch.cuda.synchronize()
            assert torch.equal(grad.cpu(), R.reduce(ref, layout, accumulate_into=base).to(torch.float32)), ("accumulate", nsplit, ntaps)
            assert torch.equal(store, before), "the caller's slabs were written"


@pytest.mark.parametrize("group", [8, 16])
def test_wgrad_fold_is_exact(dev, group):
    """insar_wgrad_fold alone, with full and ragged last groups; the slabs behind nsplit are not read."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    co, ci, ntaps = 64, 64, 4
    for nsplit in (1, group - 1, group, group + 1, 3 * group, 6 * group + 1):
        store, part, ref = _slabs(dev, nsplit, nsplit, ntaps, co, ci, 0)
        before = store.clone()
        groups = -(-nsplit // group)
        out = torch.full((groups, ntaps, co, ci), NAN, device=dev)
        call("insar_wgrad_fold", ptr(part), ptr(out), ntaps * co * ci, nsplit, group, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), R.fold(ref, group).to(torch.float32)), nsplit
        assert torch.equal(store, before)


@pytest.mark.parametrize("co,ci,off", _SHAPES)
@pytest.mark.parametrize("layout", [0, 1])
def test_wgrad_finish_across_its_fold_thresholds(dev, co, ci, off, layout):
    """Ctx.wgrad_finish: at most 48 slabs the reduce kernel folds alone, 49..96 go through groups of 8, more through groups
    of 16 — each with full and ragged last groups, up to the cost model's 256 splits. insar_wgrad_fold reads its input as
    float4 (16-byte aligned slabs, a whole number of float4 each): the unaligned row stops at 48 splits."""
    from insar_unet_ca_amd import engine
    ctx = engine.Ctx(dev, torch.float32)
    shape = (co, ci) if layout == 0 else (ci, co)
    for nsplit in (48, 49, 95, 96, 97, 100, 256):
        for ntaps in (1, 4, 9, 12):
            slab = ntaps * co * ci
            if nsplit * slab > _MAX_FLOATS or (nsplit > 48 and (slab % 4 or off)):       # insar_wgrad_fold: 16-byte slabs only
                continue
            store, part, ref = _slabs(dev, nsplit * 7 + ntaps, nsplit, ntaps, co, ci, off)
            before = store.clone()
            grad = torch.full(shape + (ntaps,), NAN, device=dev)
            ctx.wgrad_finish(part, grad, nsplit, ntaps, co, ci, layout)
            torch.cuda.synchronize()
            assert not bool(torch.isnan(grad).any())
            assert torch.equal(grad.cpu(), R.reduce(ref, layout).to(torch.float32)), (nsplit, ntaps)
            assert torch.equal(store, before), "the caller's slabs were written"


# ---- column sums --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 200, 256, 257, 1000])          # two-stage above 256 rows
@pytest.mark.parametrize("cols", [64, 130])
def test_colsum_ld_is_exact(dev, rows, cols):
    """insar_colsum_ld with ld = cols and ld = 2*cols (the transposed convs' bias gradient: the first half of (sum, sum of
    squares) rows), 1 and 3 segments, from a non-zero float offset, overwrite and accumulate."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    tmp = torch.full((-(-rows // 128) * 3 * cols + 64,), NAN, device=dev)
    for segments in (1, 3):
        for ld in (cols, 2 * cols):
            for off in (0, 5):
                n = segments * rows * ld
                ref = _ints(rows + cols + segments + ld + off, -1000, 1000, n)
                store = torch.full((off + n,), _JUNK, device=dev)
                store[off:] = ref.to(torch.float32)
                want = R.colsum(ref, segments, rows, cols, ld=ld)
                assert float(want.abs().max()) < 2 ** 24
                for accumulate in (0, 1):
                    base = _ints(7 + accumulate, -500, 500, segments, cols)
                    out = base.to(torch.float32).to(dev) if accumulate else torch.full((segments, cols), NAN, device=dev)
                    call("insar_colsum_ld", ptr(store) + 4 * off, ptr(out), segments, rows, cols, ld, accumulate, ptr(tmp),
                         tmp.numel(), _lib.stream_ptr())
                    torch.cuda.synchronize()
                    exp = (base + want) if accumulate else want
                    assert torch.equal(out.cpu(), exp.to(torch.float32)), (segments, ld, off, accumulate)


@pytest.mark.parametrize("rows,rps", [(200, 64), (257, 128), (1000, 7), (1000, 128), (64, 64), (5, 8)])
@pytest.mark.parametrize("cols", [64, 130])
def test_colsum_partial_is_exact(dev, rows, rps, cols):
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    ref = _ints(rows + rps + cols, -1000, 1000, rows, cols)
    part = ref.to(torch.float32).to(dev)
    out = torch.full((-(-rows // rps), cols), NAN, device=dev)
    call("insar_colsum_partial", ptr(part), ptr(out), rows, cols, rps, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), R.colsum_partial(ref, rows, cols, rps).to(torch.float32))
