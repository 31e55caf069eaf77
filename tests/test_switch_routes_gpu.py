"""GPU: the engine's own arithmetic around a NON-DEFAULT convolution kernel, held to exact integers.

tests/test_conv3x3_exact_gpu.py launches each 3x3 kernel with flags it chooses itself. Here the flags, the route, the rows of
the statistics slab and the choice whether a producer GEMM may write a consumer's BatchNorm-backward sums are the engine's
(ConvBN._route, _rows_flags, _flat_flags, Route.stat_rows, Route.sums_slab), under every value of the INSAR_* switches and
library knobs that select between convolution kernels. One engine.ConvBN per run, the operands of tests/conv_ref.py (small
integers: every summation order is exact, asserted by the generator and, per shape, by tests/test_conv_ref_host.py):

 * forward_conv(training=True): y equals the reference, its halo is zero; the statistics slab — NaN-prefilled, two rows
   longer than Route.stat_rows says — has every row below that written, sums to (sum y, sum y^2) exactly, and the rows
   beyond are bitwise as filled;
 * mean, invstd, scale, shift after _bn_finalize are BITWISE what the default run gives;
 * engine._dgrad without a consumer and with one that asks for its BatchNorm-backward sums: dx equals the reference, halo
   zero; the consumer's slab (zero rows as the engine allocates them, two NaN rows behind) sums to
   (sum dx*mask, sum dx*mask*yv) exactly and the rows behind are untouched; where the route cannot take the sums the
   consumer is not told that they are there.

Every case first proves from the launch record (tests/helpers.record_calls) or from unit.fwd / unit.bwd that it LEFT the
default path: a switch that changes nothing at the case's shape fails the case. Shapes come from the library's own
queries and the device's CU count. Nothing here skips."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from tests import conv_ref as R
from tests.helpers import record_calls
from tests.test_conv3x3_exact_gpu import _act, _check_slab, _desc, _equal_ints, _halo_is_zero, _same_bits

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
_KNOBS = ("igemm_xwide_min", "igemm_wide_min", "c64_grid_bwd")
SEED = R.SWITCH_SEED
_CONVS = ("insar_igemm", "insar_conv3x3_flat", "insar_conv3x3_flat_bstat", "insar_conv3x3_c64", "insar_conv3x3_c64_bstat")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()                      # fail loudly if the extension is missing
    return torch.device("cuda:0")


# ---- operands: one reference per (layer, shape), left unchanged ----------------------------------------------------------------
_OPS = {}


def _ops(dev, cin, cout, shape):
    key = (cin, cout, tuple(shape))
    assert key in R.SWITCH_ROUTE_LAYERS, f"{key}: list the shape in conv_ref.SWITCH_ROUTE_LAYERS (the host test asserts its exactness bounds)"
    if key not in _OPS:
        while len(_OPS) >= 2:
            _OPS.pop(next(iter(_OPS)))
        _OPS[key] = R.switch_operands(dev, cin, cout, shape)
    return _OPS[key]


def _consumer(ctx, o, dx_like, dtype, dev, rows_total):
    """A BNUnit that stands where the unit consuming dx stands: y = yv with dx's layout, integer scale / shift, and a slab of
    its own with two NaN rows behind the rows the engine would allocate (BNUnit.bstat_slab keeps a slab of the right size)."""
    from insar_unet_ca_amd import engine
    u = engine.BNUnit()
    u.ctx, u.x, u.cout = ctx, dx_like, dx_like.c_len
    u.y = _act(o.yv, dtype, dev)
    u.scale, u.shift = o.cscale.float().contiguous(), o.cshift.float().contiguous()
    B = dx_like.B
    rows = -(-rows_total // B)
    u.bred = torch.cat([torch.zeros((B * rows, 2, u.cout), device=dev), torch.full((2, 2, u.cout), NAN, device=dev)])
    u.bred_rows, u.bred_ready, u.bred_plain, u._mask_off = rows, False, False, None
    return u


def _modules(dev, o):
    """Conv2d with the integer weights and a seeded bias, BatchNorm2d with seeded gamma / beta: equal in every run."""
    cout, cin = o.w.shape[:2]
    gen = torch.Generator().manual_seed(SEED + 2)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(dev)
    bn = torch.nn.BatchNorm2d(cout).to(dev)
    with torch.no_grad():
        conv.weight.copy_(o.w.float())
        conv.bias.copy_(torch.randn(cout, generator=gen))
        bn.weight.copy_(torch.rand(cout, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(cout, generator=gen))
    return conv, bn


def _run(dev, monkeypatch, dtype, o, what):
    """One ConvBN under the switches as they stand: the checks of the module docstring. Returns the unit, the launch
    records of the three stages, the coefficients and whether the consumer's sums came out of the input-gradient launch."""
    from insar_unet_ca_amd import engine
    cout, cin = o.w.shape[:2]
    B, _, H, W = o.x.shape
    ctx = engine.Ctx(dev, dtype)
    conv, bn = _modules(dev, o)
    xa = _act(o.x, dtype, dev)
    unit = engine.ConvBN(ctx, conv, bn, xa, "unit")
    rows = unit.fwd.stat_rows(xa, unit.y)
    assert rows == unit.stat_rows >= 1 and tuple(unit.stats.shape) == (rows, 2, cout), what
    slab = torch.full((rows + 2, 2, cout), NAN, device=dev)
    unit.stats = slab
    if not unit.stat_rps:
        unit.sums = slab
    else:
        unit.sums.fill_(NAN)
    log = record_calls(monkeypatch, [engine])
    unit.forward_conv(True)
    torch.cuda.synchronize()
    fwd_log = list(log)
    _equal_ints(unit.y.nchw(), o.y, what + " y")
    assert _halo_is_zero(unit.y), what + " y halo"
    _check_slab(slab, rows, o.y, what)
    coefs = {k: getattr(unit, k).clone() for k in ("mean", "invstd", "scale", "shift")}
    assert all(bool(torch.isfinite(v).all()) for v in coefs.values()), what + " coefficients"
    bwd_logs, fused = [], None
    for with_consumer in (False, True):
        tag = what + (" dgrad with a consumer" if with_consumer else " dgrad")
        ga = _act(o.g, dtype, dev)
        dxa = engine.Act.alloc(B, H, W, cin, dtype, dev)
        cons = _consumer(ctx, o, dxa, dtype, dev, unit.bwd.stat_rows(ga, dxa, 1)) if with_consumer else None
        del log[:]
        engine._dgrad(unit.bwd, ga, dxa, unit.w.dgrad, cons, False)
        torch.cuda.synchronize()
        bwd_logs.append(list(log))
        _equal_ints(dxa.nchw(), o.dx, tag + " dx")
        assert _halo_is_zero(dxa), tag + " dx halo"
        if cons is not None:
            fused = cons.bred_ready
            n = B * cons.bred_rows
            assert _same_bits(cons.bred[n:], torch.full_like(cons.bred[n:], NAN)), tag + ": rows behind the consumer's slab were written"
            body = cons.bred[:n].double()
            if fused:
                tot = body.sum(0)
                assert not bool(torch.isnan(body).any()), tag
                assert torch.equal(tot[0], o.b1.double()), f"{tag}: sum dx*mask, {int((tot[0] != o.b1.double()).sum())} channels differ"
                assert torch.equal(tot[1], o.b2.double()), f"{tag}: sum dx*mask*yv, {int((tot[1] != o.b2.double()).sum())} channels differ"
            else:
                assert not bool(body.any()), tag + ": a launch without the sums wrote the consumer's slab"
    return SimpleNamespace(unit=unit, fwd=fwd_log, bwd=bwd_logs[0], bwd_sums=bwd_logs[1], coefs=coefs, fused=fused, rows=rows)


def _names(log):
    return [n for n, _, _ in log]


def _convs(log):
    """The convolution launches of a record (queries, weight re-layouts and the BatchNorm tail left out)."""
    return [n for n, _, _ in log if n in _CONVS]


def _flags(log, name="insar_conv3x3_flat"):
    """flip bits of the launches of the flat / 64 -> 64 entry points (the fourth argument), the _bstat forms included."""
    return [a[3] for n, a, _ in log if n in (name, name + "_bstat")]


def _same_coefs(a, b, what):
    for k in a.coefs:
        assert _same_bits(a.coefs[k], b.coefs[k]), f"{what}: {k} is not bitwise the default run's"


def _set(monkeypatch, **switches):
    from insar_unet_ca_amd import engine
    for k, v in switches.items():
        assert hasattr(engine, k), k
        monkeypatch.setattr(engine, k, v)


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---- shapes from the library's queries -----------------------------------------------------------------------------------------
def _flat_batch(cin, cout, dtype, hw=128):
    """Smallest batch of hw x hw images the flat route takes in both directions, with more tiles than a persistent grid."""
    from insar_unet_ca_amd._lib import call
    for B in range(1, 17):
        d = _desc((B, hw, hw), cin, dtype)
        if call("insar_conv3x3_flat_ok", d, cout) == 1 and call("insar_conv3x3_flat_ok", d, cin) == 1:
            return B
    raise AssertionError(f"no batch up to 16 of {hw} x {hw} images reaches the flat route")


def _two_group_rows_batch(dev, cin, cout, hw=128):
    """Smallest batch of hw x hw images at which _rows_flags hands the layer to the two-work-group kernel's row tiles in
    place of the per-tap kernel's 256 x 256 tiles."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    for B in range(1, 33):
        M = B * hw * hw
        d = _desc((B, hw, hw), cin, BF16)
        if ((M // 256) * (cout // 128) >= 2 * _cus(dev) and call("insar_conv3x3_flat2_rows_ok", d, cout) == 1
                and call("insar_conv3x3_flat_ok", d, cout) == 0
                and call("insar_igemm_tile_cols_dt", M, cout, _lib.BF16) == 256):
            return B
    raise AssertionError("no batch up to 32 reaches the two-work-group row tiles")


# ---- INSAR_C64, BSTAT_C64, c64_grid_bwd -----------------------------------------------------------------------------------------
_C64_SHAPE = (3, 30, 30)


@pytest.mark.parametrize("mode,kinds", [("0", ("igemm", "igemm")), ("fwd", ("c64", "igemm")), ("bwd", ("igemm", "c64"))])
def test_insar_c64(dev, monkeypatch, mode, kinds):
    """INSAR_C64 = 0 / fwd / bwd (read when the unit is built): the 64 -> 64 kernel in neither / one direction, the per-tap
    GEMM in the other, against the default (both directions on the 64 -> 64 kernel)."""
    o = _ops(dev, 64, 64, _C64_SHAPE)
    monkeypatch.delenv("INSAR_C64", raising=False)
    base = _run(dev, monkeypatch, BF16, o, "INSAR_C64 default")
    assert (base.unit.fwd.kind, base.unit.bwd.kind) == ("c64", "c64")
    assert "insar_conv3x3_c64" in _names(base.fwd) and "insar_conv3x3_c64_bstat" in _names(base.bwd_sums) and base.fused
    monkeypatch.setenv("INSAR_C64", mode)
    var = _run(dev, monkeypatch, BF16, o, f"INSAR_C64={mode}")
    assert (var.unit.fwd.kind, var.unit.bwd.kind) == kinds
    assert ("insar_igemm" in _names(var.fwd)) == (kinds[0] == "igemm") and ("insar_conv3x3_c64" in _names(var.fwd)) == (kinds[0] == "c64")
    assert ("insar_igemm" in _names(var.bwd)) == (kinds[1] == "igemm") and ("insar_conv3x3_c64" in _names(var.bwd)) == (kinds[1] == "c64")
    assert var.fused, "the per-tap GEMM and the 64 -> 64 kernel both take a consumer's sums"
    _same_coefs(var, base, f"INSAR_C64={mode}")


def test_bstat_c64_off(dev, monkeypatch):
    """BSTAT_C64 = 0: the 64 -> 64 input-gradient launch leaves the consumer's sums to a pass of their own."""
    o = _ops(dev, 64, 64, _C64_SHAPE)
    base = _run(dev, monkeypatch, BF16, o, "BSTAT_C64 default")
    assert base.fused and _convs(base.bwd_sums) == ["insar_conv3x3_c64_bstat"]
    _set(monkeypatch, BSTAT_C64=False)
    var = _run(dev, monkeypatch, BF16, o, "BSTAT_C64=0")
    assert var.unit.bwd.kind == "c64" and not var.fused and _convs(var.bwd_sums) == ["insar_conv3x3_c64"]
    _same_coefs(var, base, "BSTAT_C64=0")


def test_knob_c64_grid_bwd(dev, monkeypatch):
    """c64_grid_bwd = 0 (one work-group per CU) and a grid below the tile count: every work-group of the input-gradient
    launch walks several tiles; the slab keeps its rows, the ones the smaller grid does not write stay zero."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    o = _ops(dev, 64, 64, _C64_SHAPE)
    geo = (C.c_int32 * 6)()
    assert call("insar_conv3x3_c64_geometry", _desc(_C64_SHAPE, 64, BF16), C.addressof(geo)) == 1
    ntiles = geo[4]
    grid = max(2, ntiles // 3)
    assert 0 < grid < ntiles <= _cus(dev)
    before = _lib.tune("c64_grid_bwd")
    assert before == 0
    try:
        base = _run(dev, monkeypatch, BF16, o, "c64_grid_bwd=0")
        assert base.rows == ntiles and _convs(base.bwd_sums) == ["insar_conv3x3_c64_bstat"]
        _lib.tune("c64_grid_bwd", grid)
        assert _lib.tune("c64_grid_bwd") == grid
        var = _run(dev, monkeypatch, BF16, o, f"c64_grid_bwd={grid}")
        assert var.rows == ntiles and var.fused and _convs(var.bwd_sums) == ["insar_conv3x3_c64_bstat"]
        _same_coefs(var, base, f"c64_grid_bwd={grid}")
    finally:
        _lib.tune("c64_grid_bwd", before)
    assert _lib.tune("c64_grid_bwd") == before


# ---- FLAT_ROWS ---------------------------------------------------------------------------------------------------------------------
def test_flat_rows_off(dev, monkeypatch):
    """FLAT_ROWS = 0: the per-tap GEMM where the default is the 8-wave kernel's row tiles (64-column tiles on this grid)."""
    from insar_unet_ca_amd._lib import call
    shape = (2, 16, 32)
    assert call("insar_conv3x3_flat_rows_ok", _desc(shape, 128, BF16), 128) == 1
    o = _ops(dev, 128, 128, shape)
    base = _run(dev, monkeypatch, BF16, o, "FLAT_ROWS default")
    assert (base.unit.fwd.kind, base.unit.bwd.kind) == ("rows", "rows") and base.unit.fwd.geo & 8 and not base.unit.fwd.geo & 32
    assert all(f & 8 for f in _flags(base.fwd) + _flags(base.bwd)) and len(_flags(base.fwd)) == 1
    assert base.rows == 2 * 16 * 32 // 256
    _set(monkeypatch, FLAT_ROWS=False)
    var = _run(dev, monkeypatch, BF16, o, "FLAT_ROWS=0")
    assert (var.unit.fwd.kind, var.unit.bwd.kind) == ("igemm", "igemm")
    assert _names(var.fwd).count("insar_igemm") == 1 and not _flags(var.fwd) and _convs(var.bwd) == ["insar_igemm"]
    assert var.rows == call("insar_igemm_num_mtiles", 2 * 16 * 32, 128)
    _same_coefs(var, base, "FLAT_ROWS=0")


# ---- the flat route: FLAT2, FLAT2_PERSIST, FLAT_PP, FLAT_PERSIST, STAT_PREFOLD_ROWS ----------------------------------------------
def _flat_case(dev, dtype):
    cin, cout = 64, 128
    shape = (_flat_batch(cin, cout, dtype), 128, 128)
    return _ops(dev, cin, cout, shape), shape


def _one_flag(log, what):
    f = _flags(log)
    assert len(f) == 1, f"{what}: {_names(log)}"
    return f[0]


@pytest.mark.parametrize("value", [0, 2, 3])
def test_flat2(dev, monkeypatch, value):
    """FLAT2 = 0 (the 8-wave kernel), 2 (two work-groups, flat geometry, one work-group per tile), 3 (flat geometry,
    persistent) against the default 1 (its row tiles on a 128-pixel-wide grid)."""
    from insar_unet_ca_amd._lib import call
    o, shape = _flat_case(dev, BF16)
    assert call("insar_conv3x3_flat2_rows_ok", _desc(shape, 64, BF16), 64) == 1
    base = _run(dev, monkeypatch, BF16, o, "FLAT2 default")
    assert (base.unit.fwd.kind, base.unit.bwd.kind) == ("flat", "flat")
    f0, b0 = _one_flag(base.fwd, "default"), _one_flag(base.bwd, "default")
    assert f0 & 32 and f0 & 8 and f0 & 4 and b0 & 32 and b0 & 8 and b0 & 1 and not b0 & 4
    _set(monkeypatch, FLAT2=value)
    var = _run(dev, monkeypatch, BF16, o, f"FLAT2={value}")
    f, b = _one_flag(var.fwd, "variant"), _one_flag(var.bwd, "variant")
    bs = _one_flag(var.bwd_sums, "variant with sums")
    assert "insar_conv3x3_flat_bstat" in _names(var.bwd_sums) and var.fused and bs == b
    if value == 0:
        assert not f & 32 and not f & 8 and f & 4 and not b & 32 and b & 4
        assert var.rows == min(call("insar_conv3x3_flat_num_mtiles", _desc(shape, 64, BF16)), _cus(dev) & ~7)
    elif value == 2:
        assert f & 32 and not f & 8 and not f & 4 and b & 32 and not b & 12
        assert var.rows == call("insar_conv3x3_flat_num_mtiles", _desc(shape, 64, BF16))
    else:
        assert f & 32 and not f & 8 and f & 4 and b & 32 and not b & 12
    assert var.rows == call("insar_conv3x3_flat_stat_rows", _desc(shape, 64, BF16), 128, f)
    _same_coefs(var, base, f"FLAT2={value}")


@pytest.mark.parametrize("value", [0, 2])
def test_flat2_persist(dev, monkeypatch, value):
    """FLAT2_PERSIST = 0 (never) and 2 (input gradients too) against the default 1 (forward launches only)."""
    o, shape = _flat_case(dev, BF16)
    base = _run(dev, monkeypatch, BF16, o, "FLAT2_PERSIST default")
    _set(monkeypatch, FLAT2_PERSIST=value)
    var = _run(dev, monkeypatch, BF16, o, f"FLAT2_PERSIST={value}")
    f, b, bs = _one_flag(var.fwd, "fwd"), _one_flag(var.bwd, "bwd"), _one_flag(var.bwd_sums, "bwd with sums")
    assert f & 32 and b & 32 and bs == b
    assert bool(f & 4) == (value == 2) and bool(b & 4) == (value == 2)
    assert (f, b) != (_one_flag(base.fwd, "fwd"), _one_flag(base.bwd, "bwd"))
    assert var.fused
    _same_coefs(var, base, f"FLAT2_PERSIST={value}")


def _eight_wave(monkeypatch, dtype):
    if dtype == BF16:            # bf16 takes the two-work-group kernel by default: these switches belong to the 8-wave one
        _set(monkeypatch, FLAT2=0)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_flat_pp_off(dev, monkeypatch, dtype):
    """FLAT_PP = 0: the 8-wave flat kernel's plain tap loop (fp32; bf16 with FLAT2 = 0) against the default."""
    o, shape = _flat_case(dev, dtype)
    base = _run(dev, monkeypatch, dtype, o, "FLAT_PP default")
    _eight_wave(monkeypatch, dtype)
    near = _run(dev, monkeypatch, dtype, o, "FLAT_PP default on the 8-wave kernel") if dtype == BF16 else base
    _set(monkeypatch, FLAT_PP=0)
    var = _run(dev, monkeypatch, dtype, o, "FLAT_PP=0")
    f, b = _one_flag(var.fwd, "fwd"), _one_flag(var.bwd, "bwd")
    assert var.unit.fwd.kind == "flat" and not f & 2 and not b & 2 and not f & 32 and not b & 32
    # the run that differs in FLAT_PP alone has the ping-pong bit and no other difference
    assert _one_flag(near.fwd, "fwd") == f | 2 and _one_flag(near.bwd, "bwd") == b | 2
    _same_coefs(var, near, "FLAT_PP=0 against the 8-wave default")
    assert var.fused
    _same_coefs(var, base, "FLAT_PP=0")


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_flat_persist(dev, monkeypatch, dtype, value):
    """FLAT_PERSIST = 0 (one work-group per tile) and 1 (persistent forward launches only) against the default 2: the
    statistics slab has one row per tile instead of one per work-group."""
    from insar_unet_ca_amd._lib import call
    o, shape = _flat_case(dev, dtype)
    mtiles = call("insar_conv3x3_flat_num_mtiles", _desc(shape, 64, dtype))
    assert mtiles > (_cus(dev) & ~7), "the shape must give a persistent grid something to carry"
    base = _run(dev, monkeypatch, dtype, o, "FLAT_PERSIST default")
    _eight_wave(monkeypatch, dtype)
    near = _run(dev, monkeypatch, dtype, o, "FLAT_PERSIST default on the 8-wave kernel") if dtype == BF16 else base
    _set(monkeypatch, FLAT_PERSIST=value)
    var = _run(dev, monkeypatch, dtype, o, f"FLAT_PERSIST={value}")
    f, b = _one_flag(var.fwd, "fwd"), _one_flag(var.bwd, "bwd")
    assert not f & 32 and bool(f & 4) == (value == 1) and not b & 4
    assert var.rows == (mtiles if value == 0 else _cus(dev) & ~7)
    # the run that differs in FLAT_PERSIST alone is persistent in both directions and differs in that bit only
    assert _one_flag(near.fwd, "fwd") == f | 4 and _one_flag(near.bwd, "bwd") == b | 4 and near.rows == _cus(dev) & ~7
    _same_coefs(var, near, f"FLAT_PERSIST={value} against the 8-wave default")
    assert var.fused
    _same_coefs(var, base, f"FLAT_PERSIST={value}")


def test_stat_prefold_rows(dev, monkeypatch):
    """STAT_PREFOLD_ROWS below the slab's rows: insar_colsum_partial folds the slab before insar_bn_finalize."""
    o, shape = _flat_case(dev, F32)
    base = _run(dev, monkeypatch, F32, o, "STAT_PREFOLD_ROWS default")
    assert "insar_colsum_partial" not in _names(base.fwd) and base.rows > 128
    _set(monkeypatch, STAT_PREFOLD_ROWS=100)
    var = _run(dev, monkeypatch, F32, o, "STAT_PREFOLD_ROWS=100")
    assert var.rows == base.rows and var.unit.stat_rps == 64 and var.unit.fold_rows == -(-var.rows // 64) > 1
    names = _names(var.fwd)
    assert names.count("insar_colsum_partial") == 1 and names.index("insar_colsum_partial") < names.index("insar_bn_finalize")
    (args,) = [a for n, a, _ in var.fwd if n == "insar_colsum_partial"]
    assert args[2:5] == (var.rows, 2 * 128, 64)
    assert not bool(torch.isnan(var.unit.sums).any()), "a row of the pre-folded slab was not written"
    _same_coefs(var, base, "STAT_PREFOLD_ROWS=100")


# ---- FLAT2_KMAX (and FLAT2 = 0) where the per-tap kernel would run 256 x 256 tiles ---------------------------------------------
@pytest.mark.parametrize("which", ["kmax-0", "kmax-below-K", "flat2-0"])
def test_flat2_kmax(dev, monkeypatch, which):
    """A 128 -> 256 layer on the smallest grid with two 128-column tiles per CU slot pair: by default the two-work-group
    kernel's row tiles, with FLAT2_KMAX = 0 or just below the layer's 128 input channels (or FLAT2 = 0) the per-tap kernel's
    256 x 256 tiles."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    cin, cout = 128, 256
    shape = (_two_group_rows_batch(dev, cin, cout), 128, 128)
    M = shape[0] * shape[1] * shape[2]
    o = _ops(dev, cin, cout, shape)
    base = _run(dev, monkeypatch, BF16, o, "FLAT2_KMAX default")
    assert base.unit.fwd.kind == "rows" and base.unit.fwd.geo & 40 == 40 and _one_flag(base.fwd, "fwd") & 40 == 40
    assert base.rows == call("insar_conv3x3_flat_stat_rows", _desc(shape, cin, BF16), cout, base.unit.fwd.geo)
    _set(monkeypatch, **{"kmax-0": dict(FLAT2_KMAX=0), "kmax-below-K": dict(FLAT2_KMAX=cin - 1), "flat2-0": dict(FLAT2=0)}[which])
    var = _run(dev, monkeypatch, BF16, o, which)
    assert var.unit.fwd.kind == "igemm" and _names(var.fwd).count("insar_igemm") == 1 and not _flags(var.fwd)
    assert call("insar_igemm_tile_cols_dt", M, cout, _lib.BF16) == 256 and call("insar_igemm_tile_rows", M, cout) == 256
    assert var.rows == call("insar_igemm_num_mtiles", M, cout) == M // 256
    _same_coefs(var, base, which)


# ---- the per-tap GEMM's tile knobs ---------------------------------------------------------------------------------------------
def _with_knobs(dev, monkeypatch, o, dtype, M, N, settings, want_cols, what):
    """Runs under the knob settings; the tile the library reports for (M, N) must be want_cols wide on 256 rows."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    before = {k: _lib.tune(k) for k in settings}
    try:
        for k, v in settings.items():
            _lib.tune(k, v)
            assert _lib.tune(k) == v
        assert call("insar_igemm_tile_rows", M, N) == 256 and call("insar_igemm_tile_cols_dt", M, N, _lib.dtype_code(dtype)) == want_cols, what
        res = _run(dev, monkeypatch, dtype, o, what)
    finally:
        for k, v in before.items():
            _lib.tune(k, v)
    for k, v in before.items():
        assert _lib.tune(k) == v
    return res


def _igemm_N(log):
    return [a[0]._obj.N for n, a, _ in log if n == "insar_igemm"]


def test_knobs_igemm_wide_tiles_lowered(dev, monkeypatch):
    """igemm_xwide_min / igemm_wide_min = 1 at a few thousand pixels: the 256 x 256 and the 256 x 128 tiles where the
    default runs 256 x 64 tiles, both directions of a 256 -> 256 layer."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    shape, c = (2, 60, 72), 256
    M = shape[0] * shape[1] * shape[2]
    o = _ops(dev, c, c, shape)
    assert call("insar_igemm_tile_rows", M, c) == 256 and call("insar_igemm_tile_cols_dt", M, c, _lib.BF16) == 64
    base = _run(dev, monkeypatch, BF16, o, "wide tiles default")
    assert (base.unit.fwd.kind, base.unit.bwd.kind) == ("igemm", "igemm") and _igemm_N(base.fwd) == [c] and _igemm_N(base.bwd) == [c]
    for settings, cols in (({"igemm_xwide_min": 1}, 256), ({"igemm_wide_min": 1}, 128)):
        var = _with_knobs(dev, monkeypatch, o, BF16, M, c, settings, cols, f"{settings}")
        assert var.unit.fwd.kind == "igemm" and _igemm_N(var.fwd) == [c] and _igemm_N(var.bwd_sums) == [c] and var.fused
        assert var.rows == base.rows == call("insar_igemm_num_mtiles", M, c)
        _same_coefs(var, base, f"{settings}")


def test_knobs_igemm_wide_tiles_raised(dev, monkeypatch):
    """igemm_xwide_min raised: the 256-column tile is refused and the 128-column one runs; igemm_wide_min raised as well: 64
    columns — on a 64 -> 256 layer whose grid (130 pixels wide: no row tiles) takes 256 x 256 tiles by default."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    cin, cout = 64, 256
    B = next(b for b in range(1, 17) if call("insar_igemm_tile_cols_dt", b * 128 * 130, cout, _lib.BF16) == 256)
    shape = (B, 128, 130)
    M = B * 128 * 130
    o = _ops(dev, cin, cout, shape)
    base = _run(dev, monkeypatch, BF16, o, "wide tiles default")
    assert base.unit.fwd.kind == "igemm" and _igemm_N(base.fwd) == [cout]
    big = 1 << 30
    for settings, cols in (({"igemm_xwide_min": big}, 128), ({"igemm_xwide_min": big, "igemm_wide_min": big}, 64)):
        var = _with_knobs(dev, monkeypatch, o, BF16, M, cout, settings, cols, f"{settings}")
        assert var.unit.fwd.kind == "igemm" and _igemm_N(var.fwd) == [cout] and var.rows == base.rows
        _same_coefs(var, base, f"{settings}")


# ---- nothing leaks ---------------------------------------------------------------------------------------------------------------
def test_no_knob_leaks(dev):
    """Last in the file: every knob this file sets reads 0 again."""
    from insar_unet_ca_amd import _lib
    for k in _KNOBS:
        assert _lib.tune(k) == 0, k
