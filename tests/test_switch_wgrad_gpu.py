"""GPU: engine._wgrad_conv3, UpPlan.backward and deeplab.ConvUnit._weight_grad under every value of the weight-gradient
switches, held to exact integers.

tests/test_wgrad3_exact_gpu.py launches the row-of-taps kernels with an nsplit and a slab buffer it chooses itself. Here
nsplit, the slabs a work-group writes, the size of ctx.wgrad_part and the number of slabs ctx.wgrad_finish folds are the
engine's (one formula per branch of _wgrad_conv3). Operands are tests/wgrad3_ref.py's integers (x, g in {-1, 0, 1}: every
partial sum in any partition of the pixels is exact in fp32; tests/test_wgrad3_ref_host.py asserts the bound per shape), so
the folded gradient has ONE right answer and is compared with torch.equal.

Every run (`_run`): the slab buffer is filled with NaN right before the launch (a slab that is folded but was never
written shows in the gradient), and from the launch record (tests/helpers.record_calls)
 - the entry point is the one the case names; nsplit >= 1;
 - the buffer handed to the kernel is ctx's and holds at least nsplit * slabs * 9 * Cout * Cin floats;
 - insar_wgrad_fold / insar_wgrad_reduce folded exactly nsplit * slabs slabs.
Every case shows that it left the default path (another entry point or another nsplit than the default run's). Where a
constant does not apply by construction (a fill constant in the configuration it does not steer, a tile WGRAD_K_TILES leaves
out) the case asserts that the record is unchanged. fp32 runs exist where fp32 has the route: WGRAD_ROWS and the fill
constants; the grid cap never binds in fp32 (it fills every slot) and wgrad_tile_max is read for bf16 only.
Nothing here skips."""
from types import SimpleNamespace

import pytest
import torch

from tests import wgrad3_ref as G
from tests.helpers import record_calls
from tests.test_conv3x3_exact_gpu import _act, _desc

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
_ROW_ENTRIES = ("insar_wgrad_conv3", "insar_wgrad_conv3x", "insar_wgrad_conv3y", "insar_wgrad_conv3k")

# the layers of the cases live beside the reference; tests/test_wgrad3_ref_host.py asserts the exactness bound of each
LAYER_128, LAYER_X, LAYER_DEEP, LAYER_ODD = G.LAYER_128, G.LAYER_X, G.LAYER_DEEP, G.LAYER_ODD


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()                      # fail loudly if the extension is missing
    return torch.device("cuda:0")


_OPS = {}


def _ops(dev, layer):
    if layer not in _OPS:
        while len(_OPS) >= 2:
            _OPS.pop(next(iter(_OPS)))
        cin, cout, (B, H, W) = layer
        _OPS[layer] = G.integer_operands(G.SWITCH_SEED, B, cin, cout, H, W, device=dev)
    return _OPS[layer]


def _set(monkeypatch, **switches):
    from insar_unet_ca_amd import engine
    for k, v in switches.items():
        assert hasattr(engine, k), k
        monkeypatch.setattr(engine, k, v)


def _ctx(dev, monkeypatch, dtype, side):
    """A Ctx with or without the side stream (INSAR_SIDE_STREAM is read when it is built)."""
    from insar_unet_ca_amd import engine
    if side:
        monkeypatch.delenv("INSAR_SIDE_STREAM", raising=False)
    else:
        monkeypatch.setenv("INSAR_SIDE_STREAM", "0")
    ctx = engine.Ctx(dev, dtype)
    assert (ctx.side is not None) == side
    return ctx


def _poison_slabs(ctx, requests):
    """ctx.wgrad_part hands its buffer out all NaN (filled on the stream the kernel is about to run on)."""
    inner = ctx.wgrad_part

    def wgrad_part(floats):
        t = inner(floats)
        t.fill_(NAN)
        requests.append(floats)
        return t
    ctx.wgrad_part = wgrad_part


def _read_record(log, ctx, requests, cout, cin, ntaps, slabs, what):
    """entry, nsplit and the folded slab count from a launch record, with the checks of the module docstring."""
    kern = [(n, a) for n, a, _ in log if n in _ROW_ENTRIES + ("insar_wgrad",)]
    assert len(kern) == 1, f"{what}: {[n for n, _ in kern]}"
    entry, a = kern[0]
    if entry == "insar_wgrad":
        d = a[0]._obj
        nsplit, part = int(d.nsplit), int(d.part)
        assert int(d.ntaps) == ntaps
    else:
        nsplit, part = a[3], a[2]
    assert nsplit >= 1, what
    need = nsplit * slabs * ntaps * cout * cin
    assert part == ctx._wgrad_part.data_ptr() and ctx._wgrad_part.numel() >= need and requests == [need], \
        f"{what}: slab buffer of {ctx._wgrad_part.numel()} floats (asked for {requests}) for {need}"
    folds = [a for n, a, _ in log if n == "insar_wgrad_fold"]
    reduces = [a for n, a, _ in log if n == "insar_wgrad_reduce"]
    assert len(reduces) == 1 and len(folds) <= 1, what
    if folds:
        assert nsplit * slabs > 48 and folds[0][0] == part and folds[0][2] == ntaps * cout * cin
        folded, group = folds[0][3], folds[0][4]
        assert reduces[0][2] == -(-folded // group) and reduces[0][0] == ctx._wgrad_fold.data_ptr()
    else:
        folded = reduces[0][2]
        assert reduces[0][0] == part
    assert folded == nsplit * slabs, f"{what}: {folded} slabs folded, {nsplit} x {slabs} written"
    assert reduces[0][3:6] == (ntaps, cout, cin)
    return entry, nsplit


def _run(dev, monkeypatch, dtype, layer, side=True, what=""):
    from insar_unet_ca_amd import engine
    from insar_unet_ca_amd._lib import call
    cin, cout, shape = layer
    o = _ops(dev, layer)
    ctx = _ctx(dev, monkeypatch, dtype, side)
    xa, ga = _act(o.x, dtype, dev), _act(o.g, dtype, dev)
    grad = torch.full((cout, cin, 3, 3), NAN, device=dev)
    requests = []
    _poison_slabs(ctx, requests)
    log = record_calls(monkeypatch, [engine])
    with ctx.side_stream():
        engine._wgrad_conv3(ctx, xa, ga, grad)
    ctx.join_side()
    torch.cuda.synchronize()
    names = [n for n, _, _ in log]
    slabs = call("insar_wgrad_conv3k_slices", xa.ref, cout) if "insar_wgrad_conv3k" in names else 1
    assert slabs >= 1
    entry, nsplit = _read_record(log, ctx, requests, cout, cin, 9, slabs, what)
    bad = grad.double() != o.dw.double()
    assert not bool(bad.any()), f"{what} ({entry}, nsplit {nsplit}): {int(bad.sum())} of {bad.numel()} elements differ"
    return SimpleNamespace(entry=entry, nsplit=nsplit, slabs=slabs)


def _tile(query, layer, dtype=BF16):
    from insar_unet_ca_amd._lib import call
    cin, cout, shape = layer
    return call(query, _desc(shape, cin, dtype), cout)


# ---- which kernel: WGRAD_ROWS, WGRAD_X, WGRAD_Y, WGRAD_K -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_wgrad_rows_off(dev, monkeypatch, dtype):
    """WGRAD_ROWS = 0: the per-tap kernel (insar_wgrad) where the default is the row-of-taps kernel."""
    base = _run(dev, monkeypatch, dtype, LAYER_128, what="WGRAD_ROWS default")
    assert base.entry == "insar_wgrad_conv3" and _tile("insar_wgrad_conv3_tile", LAYER_128, dtype)
    _set(monkeypatch, WGRAD_ROWS=False)
    var = _run(dev, monkeypatch, dtype, LAYER_128, what="WGRAD_ROWS=0")
    assert var.entry == "insar_wgrad"


def test_wgrad_x_off(dev, monkeypatch):
    """WGRAD_X = 0: wgrad3's 128 x 128 tiles (six of them) where the default is the 256 x 128 six-phase kernel."""
    assert _tile("insar_wgrad_conv3x_tile", LAYER_X) == (256 << 16) | 128
    base = _run(dev, monkeypatch, BF16, LAYER_X, what="WGRAD_X default")
    assert base.entry == "insar_wgrad_conv3x"
    _set(monkeypatch, WGRAD_X=False)
    var = _run(dev, monkeypatch, BF16, LAYER_X, what="WGRAD_X=0")
    assert var.entry == "insar_wgrad_conv3" and _tile("insar_wgrad_conv3_tile", LAYER_X) == (128 << 16) | 128


@pytest.mark.parametrize("value", [1, 2, 3])
def test_wgrad_y(dev, monkeypatch, value):
    """WGRAD_Y bit 0: the 4-wave 128 x 128 kernel instead of wgrad3x (256 -> 128); bit 1: instead of wgrad3<128, 128>
    (128 -> 128). Each layer under each value; the layer a bit does not name keeps its default kernel."""
    assert _tile("insar_wgrad_conv3y_tile", LAYER_X) and _tile("insar_wgrad_conv3y_tile", LAYER_128)
    _set(monkeypatch, WGRAD_Y=value)
    seen = set()
    for layer, bit, default in ((LAYER_X, 1, "insar_wgrad_conv3x"), (LAYER_128, 2, "insar_wgrad_conv3")):
        var = _run(dev, monkeypatch, BF16, layer, what=f"WGRAD_Y={value} {layer[0]}->{layer[1]}")
        assert var.entry == ("insar_wgrad_conv3y" if value & bit else default)
        seen.add(var.entry)
    assert "insar_wgrad_conv3y" in seen


@pytest.mark.parametrize("tiles,entry", [("128x64,128x128", "insar_wgrad_conv3k"), ("128x64,64x64", "insar_wgrad_conv3")],
                         ids=["tile-included", "tile-excluded"])
def test_wgrad_k(dev, monkeypatch, tiles, entry):
    """WGRAD_K = 1 with WGRAD_K_TILES naming the layer's 128 x 128 tile (wgrad3k: KS slabs per work-group, all folded) and
    not naming it (the default kernel although WGRAD_K is set)."""
    assert _tile("insar_wgrad_conv3k_tile", LAYER_128) == (128 << 16) | 128
    _set(monkeypatch, WGRAD_K=True, WGRAD_K_TILES=set(tiles.split(",")))
    var = _run(dev, monkeypatch, BF16, LAYER_128, what=f"WGRAD_K=1 tiles {tiles}")
    assert var.entry == entry
    if entry == "insar_wgrad_conv3k":
        assert var.slabs == _tile("insar_wgrad_conv3k_slices", LAYER_128) == 2


# ---- how many work-groups: WGRAD_GRID_CAP and the fill constants -------------------------------------------------------------
def test_wgrad_grid_cap(dev, monkeypatch):
    """WGRAD_GRID_CAP = 0 (off) and a cap below the layer's 48 tiles (nsplit = max(1, 0)) against the default 200, on a
    512 -> 512 layer with WGRAD_X = 0 in all three runs (48 tiles of 128 x 128: there the default cap binds at a small grid)."""
    _set(monkeypatch, WGRAD_X=False)
    base = _run(dev, monkeypatch, BF16, LAYER_DEEP, what="WGRAD_GRID_CAP default")
    assert base.entry == "insar_wgrad_conv3" and base.nsplit == 200 // 48
    _set(monkeypatch, WGRAD_GRID_CAP=0)
    off = _run(dev, monkeypatch, BF16, LAYER_DEEP, what="WGRAD_GRID_CAP=0")
    assert off.nsplit > base.nsplit, "the default cap does not bind on this layer: pick one where it does"
    _set(monkeypatch, WGRAD_GRID_CAP=40)
    low = _run(dev, monkeypatch, BF16, LAYER_DEEP, what="WGRAD_GRID_CAP=40")
    assert low.nsplit == 1


@pytest.mark.parametrize("side", [True, False], ids=["side-stream", "no-side-stream"])
@pytest.mark.parametrize("name,layer", [("WGRAD_FILL", LAYER_X), ("WGRAD_FILL_SMALL", LAYER_128), ("WGRAD_FILL_ALONE", LAYER_128)])
def test_wgrad_fill(dev, monkeypatch, name, layer, side):
    """A fill constant at 0.25 and at 1.0, with a side stream and without. WGRAD_FILL steers wgrad3x / 3y / 3k and
    WGRAD_FILL_SMALL wgrad3 beside a side stream, WGRAD_FILL_ALONE both without one: there the two values must give
    different nsplit (one of them above the 48 slabs the re-layout kernel folds by itself); in the other configuration the
    constant must not matter."""
    applies = side != (name == "WGRAD_FILL_ALONE")
    _set(monkeypatch, WGRAD_GRID_CAP=0)        # the cap would hide the fill on these layers
    res = []
    for value in (0.25, 1.0):
        _set(monkeypatch, **{name: value})
        res.append(_run(dev, monkeypatch, BF16, layer, side=side, what=f"{name}={value}"))
    assert res[0].entry == res[1].entry == ("insar_wgrad_conv3x" if layer is LAYER_X else "insar_wgrad_conv3")
    if applies:
        assert res[0].nsplit < res[1].nsplit and res[1].nsplit > 48
    else:
        assert res[0].nsplit == res[1].nsplit


def test_wgrad_fill_alone_fp32(dev, monkeypatch):
    """fp32 fills every slot beside a side stream whatever WGRAD_FILL_SMALL says (_side_fill); without one WGRAD_FILL_ALONE
    holds for it too."""
    got = {}
    for side in (True, False):
        for value in (0.25, 1.0):
            _set(monkeypatch, WGRAD_FILL_SMALL=value, WGRAD_FILL_ALONE=value)
            got[side, value] = _run(dev, monkeypatch, F32, LAYER_128, side=side, what=f"fp32 fill {value} side {side}").nsplit
    assert got[True, 0.25] == got[True, 1.0] == got[False, 1.0] and got[False, 0.25] < got[False, 1.0]


# ---- the per-tap kernel's tile: knob wgrad_tile_max ----------------------------------------------------------------------------
def test_knob_wgrad_tile_max(dev, monkeypatch):
    """wgrad_tile_max = 128: 128 x 128 tiles (four times as many) where the per-tap kernel runs one 256 x 256 tile a tap."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call
    cin, cout, shape = LAYER_ODD
    assert _tile("insar_wgrad_conv3_tile", LAYER_ODD) == 0
    before = _lib.tune("wgrad_tile_max")
    assert before == 0
    try:
        assert call("insar_wgrad_tile_pair", cin, cout, _lib.BF16) == (256 << 16) | 256
        base = _run(dev, monkeypatch, BF16, LAYER_ODD, what="wgrad_tile_max=0")
        _lib.tune("wgrad_tile_max", 128)
        assert _lib.tune("wgrad_tile_max") == 128
        assert call("insar_wgrad_tile_pair", cin, cout, _lib.BF16) == (128 << 16) | 128
        var = _run(dev, monkeypatch, BF16, LAYER_ODD, what="wgrad_tile_max=128")
        assert base.entry == var.entry == "insar_wgrad"
    finally:
        _lib.tune("wgrad_tile_max", before)
    assert _lib.tune("wgrad_tile_max") == before


# ---- the transposed convolution: WGRAD_FILL_T -------------------------------------------------------------------------------
UP_SHAPE, UP_COUT = G.UP_SHAPE, G.UP_COUT


@pytest.mark.parametrize("side", [True, False], ids=["side-stream", "no-side-stream"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_wgrad_fill_t(dev, monkeypatch, dtype, side):
    """UpPlan.backward with WGRAD_FILL_T at 0.25 and 1.0 on integer operands (tests/test_conv_transpose_gpu.py's): dW and
    dbias equal the integer reference. The constant changes nsplit in bf16 beside a side stream and nowhere else."""
    from insar_unet_ca_amd import engine
    from tests import wgrad_ref as T
    from tests import test_conv_transpose_gpu as U
    B, cin, h, w = UP_SHAPE
    nsplits = []
    for value in (0.25, 1.0):
        _set(monkeypatch, WGRAD_FILL_T=value)
        if side:
            monkeypatch.delenv("INSAR_SIDE_STREAM", raising=False)
        else:
            monkeypatch.setenv("INSAR_SIDE_STREAM", "0")
        ctx, mod, xa, cat, up, dcat = U._plan(dev, dtype, UP_SHAPE, UP_COUT, ints=True)
        assert (ctx.side is not None) == side
        requests = []
        _poison_slabs(ctx, requests)
        log = record_calls(monkeypatch, [engine])
        sink, dx = U._backward(ctx, up, dcat, UP_COUT, UP_SHAPE, dtype, dev)
        what = f"WGRAD_FILL_T={value}"
        entry, nsplit = _read_record(log, ctx, requests, UP_COUT, cin, 4, 1, what)
        assert entry == "insar_wgrad"
        nsplits.append(nsplit)
        xi, gi = xa.nchw().long(), dcat.slice(UP_COUT, UP_COUT).nchw().long()
        assert int(xi.abs().max()) <= G.UP_X_MAX and int(gi.abs().max()) <= G.UP_G_MAX       # the bound of the host test
        _, rdw, rdb = T.conv_transpose_k2s2_backward(xi, mod.weight.detach().long(), gi)
        assert torch.equal(sink.view(mod.weight).double(), rdw.double()), what + " dW"
        assert torch.equal(sink.view(mod.bias).double(), rdb.double()), what + " dbias"
    if side and dtype == BF16:
        assert nsplits[0] < nsplits[1]
    else:
        assert nsplits[0] == nsplits[1]


# ---- DeepLabV3-CA's units: WGRAD_FILL_DL ------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [True, False], ids=["side-stream", "no-side-stream"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("layer", G.UNIT_LAYERS, ids=["1x1", "dilated"])
def test_wgrad_fill_dl(dev, monkeypatch, layer, dtype, side):
    """deeplab.ConvUnit._weight_grad of a 1x1 unit and of a 3x3 unit dilated by 2 (the per-tap kernel through tap tables)
    with WGRAD_FILL_DL at 0.25 and 1.0: the gradient equals the integer reference. The constant changes nsplit in bf16
    beside a side stream; fp32 and a Ctx without a side stream fill every slot whatever it says."""
    from insar_unet_ca_amd import deeplab, engine
    cin, cout, (B, H, W), k, dil = layer
    if layer not in _OPS:
        while len(_OPS) >= 2:
            _OPS.pop(next(iter(_OPS)))
        _OPS[layer] = G.unit_operands(G.SWITCH_SEED, layer, device=dev)
    o = _OPS[layer]
    nsplits = []
    for value in (0.25, 1.0):
        what = f"WGRAD_FILL_DL={value} {'1x1' if k == 1 else 'dilated'}"
        _set(monkeypatch, WGRAD_FILL_DL=value)
        ctx = _ctx(dev, monkeypatch, dtype, side)
        conv = torch.nn.Conv2d(cin, cout, k, padding=dil * (k // 2), dilation=dil, bias=False).to(dev)
        bn = torch.nn.BatchNorm2d(cout).to(dev)
        unit = deeplab.ConvUnit(ctx, conv, bn, _act(o.x, dtype, dev), None, True, "unit")
        assert len(unit.taps) == k * k and not unit.centre_only and unit.oob == (dil > 1)
        unit.dy = _act(o.g, dtype, dev)
        grad = torch.full((cout, cin, k, k), NAN, device=dev)
        requests = []
        _poison_slabs(ctx, requests)
        log = record_calls(monkeypatch, [engine, deeplab])
        with ctx.side_stream():
            unit._weight_grad(grad)
        ctx.join_side()
        torch.cuda.synchronize()
        entry, nsplit = _read_record(log, ctx, requests, cout, cin, k * k, 1, what)
        assert entry == "insar_wgrad"
        bad = grad.double() != o.dw.double()
        assert not bool(bad.any()), f"{what} (nsplit {nsplit}): {int(bad.sum())} of {bad.numel()} elements differ"
        nsplits.append(nsplit)
    if side and dtype == BF16:
        assert nsplits[0] < nsplits[1]
    else:
        assert nsplits[0] == nsplits[1]


# ---- nothing leaks ---------------------------------------------------------------------------------------------------------------
def test_no_knob_leaks(dev):
    """Last in the file: the knob this file sets reads 0 again."""
    from insar_unet_ca_amd import _lib
    assert _lib.tune("wgrad_tile_max") == 0
