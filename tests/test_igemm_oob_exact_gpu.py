"""GPU: the out-of-bounds variant of the per-tap implicit GEMM (csrc/igemm.hip, igemm_kernel<.., OOB = true, ..>, selected by
INSAR_IGEMM_OOB_ZERO) held ELEMENT-EXACTLY to tests/conv_ref.py's integer reference, on every tile shape insar_igemm
dispatches it to (bf16 128x64, 256x64, 256x128, 256x256; fp32 128x64, 256x64), with and without the BatchNorm-backward sums.

Operands, helpers and assertions are those of tests/test_conv3x3_exact_gpu.py (imported: `_exact`, `_ops`, `_desc`, ...):
small integers for which every result and every per-channel sum is exact in bf16 / fp32, so every comparison is torch.equal.
What this file adds to each launch (`_guarded`): the output's interior is prefilled with NaN and its halo ring with a sentinel,
the statistics slab with NaN; the launch is issued twice and both results are bit for bit the same; the ring still holds the
sentinel. `_exact` then holds y, dx and the slab (one row per M tile from insar_igemm_num_mtiles, two NaN rows behind) to the
reference, plain and as channel slices of wider buffers whose other channels must come back unchanged.

Every case asserts the tile it reached through insar_igemm_tile_rows / insar_igemm_tile_cols_dt (fp32 out-of-bounds launches:
64 columns, 256 rows where tile_rows says so): a change of the selector fails the case instead of moving it to another kernel.
The wide side of each shape is the GEMM's N in one direction only (N = 64 in the other: 128x64 tiles), so every shape runs as
64 -> wide (the forward lands on the named tile) and as wide -> 64 (the input gradient does).

  test                          what of the variant it reaches
  test_oob_tiles                bounds test, redirect and live-tap list at dilation 2, 4 (layer3 / layer4), 12, 24 (ASPP; on 32x32
                                a 256-row tile is 8 image rows: with 24 the middle tiles keep 3 of 9 taps); a 16x64 map (dy and dx
                                cannot be swapped); ragged maps (M % 256 != 0, tiles straddle images: the rows-beyond-M marker)
  test_oob_centre_tap_only      dilation 36 on 32x32 as ConvUnit issues it: one tap (0, 0), the weight pointer at tap 4 (no flag)
  test_oob_tile_without_a_live_tap   the single tap (+24, 0): three of four 256-row tiles run a K loop of zero trips; they store exact
                                zeros (bias + add where given) and exact-zero statistics rows
  test_oob_epilogue_options     bias, add, gate, bias+add+gate (the input gradient with `add` is the residual sum of deeplab.py)
  test_oob_bstat                the BS = true instantiations: the consumer's BatchNorm-backward sums, plain and over gated values
  test_oob_address_probe        names the pixel a wrong (row, tap) fetched: x carries its padded pixel index in 24 channels, one
                                identity weight per tap
  test_oob_refusals             host-side rejections; y stays NaN

No kernel had to change."""
import ctypes as C

import pytest
import torch

from tests import conv_ref as R
from tests.test_conv3x3_exact_gpu import (BF16, F32, OUT_FILL, _act, _alloc, _beside_unchanged, _desc, _equal_ints, _exact, _ops, _own,  # noqa: F401
                                          _same_bits, _weights, dev)

pytestmark = pytest.mark.gpu
RING = 5.0                  # what the output's halo ring holds while a launch runs
NAN = float("nan")
E_SHAPE, E_ARG = -1001, -1005


def _tname(dt):
    return "f32" if dt == F32 else "bf16"


def _tile(M, N, dtype):
    """(rows, cols) of the out-of-bounds launch of M x N: the selectors, and for fp32 the kernel's rule (64 columns)."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    rows = call("insar_igemm_tile_rows", M, N)
    return rows, (64 if dtype == F32 else call("insar_igemm_tile_cols_dt", M, N, _lib.dtype_code(dtype)))


def _guarded(out, slab, launch, what):
    """Issue launch() twice into `out` (an Act) with its interior NaN, its halo ring RING and the slab NaN each time: the ring
    is untouched, the two results agree bit for bit. Leaves the second result with the ring back at zero."""
    own = _own(out)
    seen = []
    for _ in range(2):
        own.fill_(RING)
        own[:, 1:-1, 1:-1] = NAN
        if slab is not None:
            slab.fill_(NAN)
        launch()
        torch.cuda.synchronize()
        ring = own.clone()
        ring[:, 1:-1, 1:-1] = RING
        assert bool((ring == RING).all()), what + ": the halo ring was written"
        seen.append((own.clone(), None if slab is None else slab.clone()))
    assert _same_bits(seen[0][0], seen[1][0]), what + ": two launches differ"
    assert slab is None or _same_bits(seen[0][1], seen[1][1]), what + ": the slabs of two launches differ"
    inner = own[:, 1:-1, 1:-1].clone()
    own.zero_()
    own[:, 1:-1, 1:-1] = inner


def _taps(dil):
    return [(ky * dil - dil, kx * dil - dil) for ky in range(3) for kx in range(3)]


def _oob_launches(cin, cout, shape, dil, fwd_kw=None, bwd_kw=None, what="oob"):
    from insar_unet_ca_amd import engine
    _, h, w = shape
    taps = _taps(dil)

    def fwd(xa, ya, wf, slab, aux):
        kw = fwd_kw(aux) if fwd_kw else {}
        _guarded(ya, slab, lambda: engine._igemm(xa, ya, wf, cout, h, w, 1, taps, 0, stats=slab, oob=True, **kw), what + " forward")

    def bwd(ga, dxa, wd, aux):
        kw = bwd_kw(aux) if bwd_kw else {}
        _guarded(dxa, None, lambda: engine._igemm(ga, dxa, wd, cin, h, w, 1, [(-a, -b) for a, b in taps], 0, oob=True, **kw),
                 what + " input gradient")
    return fwd, bwd


# ---- tile shapes x geometries ----------------------------------------------------------------------------------------------------
# name: (wide channel count, dtypes, {geometry: (B, H, W)}); the tile is that of the launch whose N is the wide side
_SQ, _NONSQ, _RAGGED = "32x32", "16x64", "ragged"
_TILE_SHAPES = {
    (128, 64): (128, (BF16, F32), {_SQ: (2, 32, 32), _NONSQ: (2, 16, 64), _RAGGED: (3, 9, 13)}),
    (256, 64): (512, (BF16, F32), {_SQ: (4, 32, 32), _NONSQ: (4, 16, 64), _RAGGED: (5, 30, 30)}),
    (256, 128): (512, (BF16,), {_SQ: (16, 32, 32), _NONSQ: (16, 16, 64), _RAGGED: (17, 30, 34)}),
    (256, 256): (2048, (BF16,), {_SQ: (8, 32, 32), _NONSQ: (8, 16, 64), _RAGGED: (9, 30, 30)}),
}
_GEOMETRIES = [(_SQ, 2), (_SQ, 4), (_SQ, 12), (_SQ, 24), (_NONSQ, 12), (_RAGGED, 12)]
_TILE_CASES = [pytest.param(tile, geo, dil, swap, dt, id=f"{tile[0]}x{tile[1]}-{geo}-d{dil}-{'dgrad' if swap else 'fwd'}-{_tname(dt)}")
               for tile, (_, dts, _) in _TILE_SHAPES.items() for geo, dil in _GEOMETRIES for swap in (False, True) for dt in dts]


@pytest.mark.parametrize("tile,geo,dil,swap,dtype", _TILE_CASES)
def test_oob_tiles(dev, tile, geo, dil, swap, dtype):
    """Forward with statistics and input gradient of a dilated 3x3 convolution, both out-of-bounds launches. swap: wide -> 64
    instead of 64 -> wide, so that the input gradient is the launch on the named tile."""
    from insar_unet_ca_amd._lib import call
    wide, _, shapes = _TILE_SHAPES[tile]
    shape = shapes[geo]
    cin, cout = (wide, 64) if swap else (64, wide)
    M = shape[0] * shape[1] * shape[2]
    want = tile if dtype == BF16 or tile[1] == 64 else (tile[0], 64)
    assert _tile(M, wide, dtype) == want, "the selectors moved this shape to another tile"
    assert _tile(M, 64, dtype) == (128, 64) or tile == (128, 64)
    if geo == _RAGGED:
        assert M % 256 and (shape[1] * shape[2]) % tile[0]          # a last partial tile, tiles that straddle images
    o = _ops(dev, cin, cout, shape, dil)
    _exact(dev, dtype, o, *_oob_launches(cin, cout, shape, dil, what=f"oob {tile} dilation {dil}"),
           call("insar_igemm_num_mtiles", M, cout), what=f"oob {tile} {geo} dilation {dil}")


# ---- single launches held to a given result ---------------------------------------------------------------------------------------
def _launch_exact(dev, dtype, xvals, w, N, shape, taps, want, what, oob=True, bias=None, add=None, gate=None, rows=None,
                  bstat=None, layouts=(None, "out")):
    """One launch of engine._igemm (x from the integers xvals, `w` a [tap][N][K] tensor or a function of it giving the pointer),
    guarded as above, in the plain and the slice form of the output: the stored result equals `want` (int64 NCHW), the channels
    beside a slice are unchanged. rows: slab rows the launch writes (two NaN rows are kept behind them); bstat: (yv, scale, shift)
    integers of the consumer. Returns the plain run's slab [rows][2][N] in float64."""
    from insar_unet_ca_amd import engine
    _, h, wd = shape
    R.assert_exact_in_bf16(want)
    first = None
    for lout in layouts:
        tag = what + (" (slice form)" if lout else "")
        xa = _act(xvals, dtype, dev, "in" if lout else None)
        ya, ywide = _alloc(shape[0], h, wd, N, dtype, dev, lout)
        aux = lambda v: None if v is None else _act(v, dtype, dev, lout)
        slab = None if rows is None else torch.full((rows + 2, 2, N), NAN, device=dev)
        kw = dict(bias=None if bias is None else bias.float(), add=aux(add), gate=aux(gate))
        if bstat is not None:
            kw["bstat"] = (aux(bstat[0]), bstat[1].float(), bstat[2].float())
        _guarded(ya, slab, lambda: engine._igemm(xa, ya, w, N, h, wd, 1, taps, 0, stats=slab, oob=oob, **kw), tag)
        _equal_ints(ya.nchw(), want, tag)
        assert ywide is None or _beside_unchanged(ya, ywide, OUT_FILL), tag + ": channels beside y were written"
        if slab is not None:
            assert _same_bits(slab[rows:], torch.full_like(slab[rows:], NAN)), tag + ": slab rows beyond the launch's were touched"
            assert not bool(torch.isnan(slab[:rows]).any()), tag + ": a slab row was not written"
            if first is None:
                first = slab[:rows].double()
            else:
                assert torch.equal(slab[:rows].double(), first), tag + ": the slab differs from the plain run's"
    return first


_TWO_SHAPES = [(64, 128, (2, 32, 32)), (512, 64, (4, 32, 32))]      # the input gradient lands on 128x64 / on 256x64 tiles


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_tname)
def test_oob_centre_tap_only(dev, dtype):
    """Dilation 36 on a 32 x 32 map: only the centre tap can reach the image, and deeplab.ConvUnit issues a one-tap launch
    (no out-of-bounds flag) with the weight pointer moved to tap 4. Held to the dilated reference, forward and input gradient;
    the same launch with the flag set gives the same bits."""
    from insar_unet_ca_amd._lib import call
    cin, cout, shape = 64, 128, (2, 32, 32)
    M = shape[0] * 32 * 32
    o = _ops(dev, cin, cout, shape, 36)
    gw = _weights(dev, dtype, o)
    es = 2 if dtype == BF16 else 4
    for oob in (False, True):
        wf, wd = gw.fwd(), gw.dgrad()
        slab = _launch_exact(dev, dtype, o.x, wf.data_ptr() + 4 * cout * cin * es, cout, shape, [(0, 0)], o.y, f"centre tap, oob={oob}",
                             oob=oob, rows=call("insar_igemm_num_mtiles", M, cout))
        s1, s2 = R.channel_stats(o.y)
        assert torch.equal(slab.sum(0)[0], s1.double()) and torch.equal(slab.sum(0)[1], s2.double())
        _launch_exact(dev, dtype, o.g, wd.data_ptr() + 4 * cout * cin * es, cin, shape, [(0, 0)], o.dx, f"centre tap dgrad, oob={oob}", oob=oob)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_tname)
@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "bias+add"])
@pytest.mark.parametrize("cout,shape,tile", [(128, (2, 32, 32), (128, 64)), (512, (4, 32, 32), (256, 64)), (2048, (8, 32, 32), (256, 256))])
def test_oob_tile_without_a_live_tap(dev, cout, shape, tile, epilogue, dtype):
    """The single tap (+24, 0) on 32 x 32: only output rows 0..7 reach the image. Every tile made of rows 8..31 has an empty
    live list, runs no K step and stores its zero accumulators: exact zeros (bias + add where given), exact-zero statistics
    rows (the sums are those of the GEMM result before bias and add)."""
    from insar_unet_ca_amd._lib import call
    if dtype == F32 and tile == (256, 256):
        tile = (256, 64)
    cin = 64
    M = shape[0] * 32 * 32
    assert _tile(M, cout, dtype) == tile
    o = _ops(dev, cin, cout, shape, 24)
    w1 = torch.zeros_like(o.w)
    w1[:, :, 2, 1] = o.w[:, :, 2, 1]                            # tap (ky, kx) = (2, 1): (+24, 0) at dilation 24
    raw = R.conv3x3(o.x, w1, 24)
    assert bool(raw[:, :, :8].any()) and not bool(raw[:, :, 8:].any())
    gen = torch.Generator().manual_seed(5)
    bias = torch.randint(-5, 6, (cout,), generator=gen, dtype=torch.int64).to(dev) if epilogue else None
    add = torch.randint(-1, 2, tuple(raw.shape), generator=gen, dtype=torch.int64).to(dev) if epilogue else None
    want = raw if not epilogue else raw + bias.reshape(1, -1, 1, 1) + add
    gw = _weights(dev, dtype, o)
    wtap = gw.fwd()[7:8].contiguous()
    rows = call("insar_igemm_num_mtiles", M, cout)
    slab = _launch_exact(dev, dtype, o.x, wtap, cout, shape, [(24, 0)], want, f"tap (+24, 0) on {tile}", bias=bias, add=add, rows=rows)
    R.assert_sums_exact_in_fp32(raw)
    per_tile = 1024 // tile[0]                                   # tiles per image; the first 256 pixels of an image are rows 0..7
    rawt = raw.permute(0, 2, 3, 1).reshape(rows, tile[0], cout).double()
    assert torch.equal(slab[:, 0], rawt.sum(1)) and torch.equal(slab[:, 1], (rawt * rawt).sum(1))
    dead = [t for t in range(rows) if (t % per_tile) * tile[0] >= 256]
    assert len(dead) == rows * 3 // 4 and not bool(slab[dead].any()), "a tile without a live tap wrote nonzero statistics"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_tname)
@pytest.mark.parametrize("option", ["bias", "add", "gate", "bias+add+gate"])
@pytest.mark.parametrize("cin,cout,shape", _TWO_SHAPES)
def test_oob_epilogue_options(dev, cin, cout, shape, option, dtype):
    """tests/test_conv3x3_exact_gpu.py::test_igemm_epilogue_options on out-of-bounds launches at dilation 12: the same integer
    ranges and the same construction of the expected values; statistics (without gate) are those of the plain convolution."""
    from insar_unet_ca_amd._lib import call
    M = shape[0] * shape[1] * shape[2]
    assert _tile(M, 128, dtype) == (128, 64) and _tile(M, 64, dtype) == (128, 64)
    assert cin != 512 or _tile(M, cin, dtype) == (256, 64)
    o = _ops(dev, cin, cout, shape, 12)
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
    R.assert_exact_in_bf16(want["y"], want["dx"])

    def kw(key):
        bias, add, gate = extra[key]
        return lambda aux: dict(bias=None if bias is None else bias.float(), add=None if add is None else aux(add),
                                gate=None if gate is None else aux(gate))
    rows = None if "gate" in option else call("insar_igemm_num_mtiles", M, cout)
    _exact(dev, dtype, o, *_oob_launches(cin, cout, shape, 12, kw("y"), kw("dx"), what=f"oob {option}"), rows, want["y"], want["dx"],
           stats_of=o.y, what=f"oob {option}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_tname)
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gate"])
@pytest.mark.parametrize("cin,cout,shape", _TWO_SHAPES + [(512, 64, (16, 32, 32)), (2048, 64, (8, 32, 32))])
def test_oob_bstat(dev, cin, cout, shape, gated, dtype):
    """The input gradient at dilation 12 with InsarBstat (the BS = true instantiations): the slab holds, per M tile, the
    consumer's sums (sum dx*mask, sum dx*mask*yv) over the values as stored — after the gate where one is given — exactly."""
    from insar_unet_ca_amd._lib import call
    M = shape[0] * shape[1] * shape[2]
    tile = _tile(M, cin, dtype)
    assert tile == {64: (128, 64), 512: (256, 64) if shape[0] == 4 or dtype == F32 else (256, 128),
                    2048: (256, 256) if dtype == BF16 else (256, 64)}[cin]
    o = _ops(dev, cin, cout, shape, 12)
    gen = torch.Generator().manual_seed(R.SWITCH_SEED + 1)
    yv = torch.randint(-1, 2, tuple(o.dx.shape), generator=gen, dtype=torch.int64).to(dev)
    scale = torch.randint(1, 3, (cin,), generator=gen, dtype=torch.int64).to(dev)
    shift = torch.randint(-1, 2, (cin,), generator=gen, dtype=torch.int64).to(dev)
    gate = torch.randint(-2, 3, tuple(o.dx.shape), generator=gen, dtype=torch.int64).to(dev) if gated else None
    want = o.dx if gate is None else torch.where(gate <= 0, torch.zeros_like(o.dx), o.dx)
    b1, b2 = R.consumer_sums(want, yv, scale, shift)
    gw = _weights(dev, dtype, o)
    rows = call("insar_igemm_num_mtiles", M, cin)
    slab = _launch_exact(dev, dtype, o.g, gw.dgrad(), cin, shape, [(-a, -b) for a, b in _taps(12)], want, f"oob bstat {tile}",
                         gate=gate, rows=rows, bstat=(yv, scale, shift))
    tot = slab.sum(0)
    assert torch.equal(tot[0], b1.double()), f"sum dx*mask: {int((tot[0] != b1.double()).sum())} channels differ"
    assert torch.equal(tot[1], b2.double()), f"sum dx*mask*yv: {int((tot[1] != b2.double()).sum())} channels differ"


# ---- the address probe -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_tname)
@pytest.mark.parametrize("shape,rows", [((2, 32, 32), 128), ((32, 32, 32), 256), ((3, 30, 34), 128)])
def test_oob_address_probe(dev, shape, rows, dtype):
    """x holds, in channels 0..23 of every pixel, the bits of its index in the padded buffer; the weights are the identity for
    ONE tap and zero for the other eight, while the launch lists all nine taps at dilation 12 (liveness is that of the real
    convolution). Then y is x shifted by that tap, or zero where the tap leaves the image: a mismatch names the output pixel,
    the tap, the tile, and which pixel was fetched instead of which."""
    from insar_unet_ca_amd import engine
    B, H, W = shape
    dil, cn = 12, 64
    M = B * H * W
    assert _tile(M, cn, dtype) == (rows, 64)
    n, h, w = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
    index = ((n * (H + 2) + h + 1) * (W + 2) + w + 1).to(dev)                     # [B][H][W], never 0 inside the image
    assert int(index.max()) < 2 ** 24
    x = torch.zeros((B, cn, H, W), dtype=torch.int64, device=dev)
    for b in range(24):
        x[:, b] = (index >> b) & 1
    xa = _act(x, dtype, dev)
    ctx = engine.Ctx(dev, dtype)
    taps = _taps(dil)
    for t, (dy, dx) in enumerate(taps):
        wt = torch.zeros((cn, cn, 3, 3), device=dev)
        wt[:, :, t // 3, t % 3] = torch.eye(cn, device=dev)
        gw = engine.GemmWeight(ctx, torch.nn.Parameter(wt), "conv3")
        ya = engine.Act.alloc(B, H, W, cn, dtype, dev)
        _guarded(ya, None, lambda: engine._igemm(xa, ya, gw.fwd(), cn, H, W, 1, taps, 0, oob=True), f"probe tap {t}")
        got = ya.nchw().to(torch.int64)
        assert torch.equal(got.double(), ya.nchw().double()) and bool(((got == 0) | (got == 1)).all()), f"tap {t}: values other than 0 / 1"
        fetched = sum(got[:, b] << b for b in range(24))
        inside = (h + dy >= 0) & (h + dy < H) & (w + dx >= 0) & (w + dx < W)
        expect = torch.where(inside.to(dev), index + dy * (W + 2) + dx, torch.zeros_like(index))
        bad = (fetched != expect) | bool(got[:, 24:].any())
        if bool(bad.any()):
            i = int(bad.reshape(-1).nonzero()[0])
            raise AssertionError(f"tap {t} ({dy:+d}, {dx:+d}): output pixel m = {i} (n, h, w = {i // (H * W)}, {i // W % H}, {i % W}), "
                                 f"tile {i // rows} row {i % rows}: fetched padded pixel {int(fetched.reshape(-1)[i])}, expected "
                                 f"{int(expect.reshape(-1)[i])} (0 = the zero pixel); {int(bad.sum())} pixels differ")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _descriptor(x, y, w, N, Ho, Wo, taps, mode=0, oob=False, add=0, gate=0, stats=0):
    from insar_unet_ca_amd import _lib
    d = _lib.InsarIgemm()
    d.x, d.y, d.w, d.stats, d.add, d.gate = x, y, w, stats, add, gate
    d.N, d.Ho, d.Wo, d.stride, d.ntaps, d.mode = N, Ho, Wo, 1, len(taps), mode
    d.flags = _lib.IGEMM_OOB_ZERO if oob else 0
    d.out_stride = 1
    for i, (dy, dx) in enumerate(taps):
        d.dy[i], d.dx[i] = dy, dx
    return d


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_tname)
def test_oob_refusals(dev, dtype):
    """What insar_igemm rejects on the host: a nonzero return that names the entry point, and a NaN-prefilled y left as it was.
    The too-tall input exists as descriptor fields only (the check precedes the launch; no such buffer is allocated)."""
    from insar_unet_ca_amd import _lib, engine
    from tests.test_forward_apply_gpu import refused
    code = _lib.dtype_code(dtype)
    B, H, W, cn = 1, 8, 8, 64
    xa = engine.Act.alloc(B, H, W, cn, dtype, dev)
    ya = engine.Act.alloc(B, H, W, cn, dtype, dev)
    ya.buf.fill_(NAN)
    other = engine.Act.alloc(B, H, W, cn, dtype, dev)
    wt = torch.zeros((9, cn, cn), dtype=dtype, device=dev)
    slab = torch.full((4, 2, cn), NAN, device=dev)
    stream = _lib.stream_ptr()
    tall = 0x3fff - 1                                            # H + 2 = 0x4000: the row marker of rows beyond M
    xt = _lib.InsarAct(xa.buf.data_ptr(), 1, tall, 1, cn, 0, cn, code, 0)
    yt = _lib.InsarAct(ya.buf.data_ptr(), 1, tall, 1, cn, 0, cn, code, 0)
    cases = [
        (E_SHAPE, _descriptor(xt, yt, wt.data_ptr(), cn, tall, 1, [(0, 0)], oob=True)),
        (E_ARG, _descriptor(xa.desc, _lib.InsarAct(ya.buf.data_ptr(), B, 2 * H, 2 * W, cn // 4, 0, cn // 4, code, 0), wt.data_ptr(), cn, H, W,
                            [(0, 0)], mode=1, add=other.buf.data_ptr())),
        (E_ARG, _descriptor(xa.desc, ya.desc, wt.data_ptr(), cn, H, W, engine._TAPS3, gate=other.buf.data_ptr(), stats=slab.data_ptr())),
        (E_SHAPE, _descriptor(xa.desc, ya.desc, wt.data_ptr(), cn, H, W, _taps(2))),
    ]
    for want, d in cases:
        refused(want, "insar_igemm", "insar_igemm", C.byref(d), stream)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ya.buf).all()) and bool(torch.isnan(slab).all())
    assert not bool(xa.buf.any()) and not bool(other.buf.any())
