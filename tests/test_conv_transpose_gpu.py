"""ConvTranspose2d(k=2, s=2) on the HIP path, launch by launch and as the plan (engine.UpPlan), elementwise against
tests/wgrad_ref.py's float64 / int64 statement of the operation (held to torch.autograd by tests/test_wgrad_ref_host.py):

 * forward: insar_igemm mode 1 through engine._igemm, scattering GEMM row (ho, wo), column (a*2+b)*Cout + co to output pixel
   (2ho+a, 2wo+b) of the upper slice of a concat buffer, at shapes that reach every tile variant the selector can give;
 * input gradient: insar_igemm mode 0, stride 2, the four taps {0,1}^2, without the bstat epilogue;
 * UpPlan.forward / .backward into a GradSink: out, dx, dW (ConvTranspose2d layout), dbias; with the one-pixel bilinear
   resize; with the weight gradient issued before and after the input gradient.

Tolerances: fp32 with integer operands is exact (every sum an integer far below 2^24). Otherwise the reference is float64
on the kernel's own operands (xa.nchw(), the GEMM-layout weight), as in test_igemm_family_against_float64, with that test's
tolerances: its KERNEL_TOL (imported) for fp32, its 6e-3 for bf16 outputs (only the output rounding remains),
KERNEL_TOL * 5 for weight and bias gradients (fp32 accumulation in both dtypes). The resize links use the TOL of
tests/test_deeplab_kernels_gpu.py (imported), as test_nhwc_bilinear_resize_and_floor_pooling does.

The float64 reference runs on the tensors' device (torch matmul in float64, none of this project's kernels): the largest
forward case has 16.7 M output elements."""
import pytest
import torch
import torch.nn.functional as F

from oracle import closed_form as cf
from tests import wgrad_ref as R
from tests.test_deeplab_kernels_gpu import TOL as RESIZE_TOL      # what test_nhwc_bilinear_resize_and_floor_pooling uses
from tests.test_parity_gpu import KERNEL_TOL

pytestmark = pytest.mark.gpu

BF16_OUT_TOL = 6e-3       # test_igemm_family_against_float64's literal for bf16 outputs ("only the output rounding remains")
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()                      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _out_tol(dtype):
    return KERNEL_TOL if dtype == F32 else BF16_OUT_TOL


def _max_rel(a, b):
    """max |a-b| / max|b| (tests.helpers.max_rel), on the tensors' device."""
    a, b = a.double(), b.double()
    den = float(b.abs().max())
    return float((a - b).abs().max()) / (den if den > 0 else 1.0)


def _ints(seed, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def _act(vals, dtype, dev):
    from insar_unet_ca_amd import engine
    b, c, h, w = vals.shape
    a = engine.Act.alloc(b, h, w, c, dtype, dev)
    engine.pack_input(vals.float().to(dev), a)
    return a


def _halo_abs(a):
    t = a.buf.float().clone()
    t[:, 1:-1, 1:-1] = 0
    return float(t.abs().max())


def _weight(ctx, cin, cout, ints, dev):
    from insar_unet_ca_amd import engine
    w = _ints(41, -2, 2, cin, cout, 2, 2).float() if ints else cf.fill_tensor("weight", (cin, cout, 2, 2), 11)
    p = torch.nn.Parameter(w.contiguous().to(dev))
    return p, engine.GemmWeight(ctx, p, "convT")


def _w_fwd(gw, cin, cout):
    """The forward GEMM operand [a*2+b][co][ci] as the kernel sees it -> (Ci, Co, 2, 2) float64."""
    return gw.fwd().double().reshape(2, 2, cout, cin).permute(3, 2, 0, 1).contiguous()


def _w_dgrad(gw, cin, cout):
    """The input-gradient GEMM operand [a*2+b][ci][co] -> (Ci, Co, 2, 2) float64."""
    return gw.dgrad().double().reshape(2, 2, cin, cout).permute(2, 3, 0, 1).contiguous()


# (B, Cin, h, w), Cout, forward tile rows, forward tile columns {dtype}: by igemm_bm_for / igemm_bn_for / igemm_xwide of
# csrc/igemm.hip at N = 4*Cout. The 128 x 128 four-wave tile is unreachable at default knobs: 128-row tiles are chosen only
# while ceil(M/256) * (N/64) < 128, the 128-column tile on them only when ceil(M/128) * (N/128) > 256, and
# ceil(M/128) * (N/128) <= 2*ceil(M/256) * (N/128) = ceil(M/256) * (N/64) < 128.
_SHAPES = [
    ((2, 128, 8, 8), 64, 128, {F32: 64, BF16: 64}),
    ((3, 64, 5, 7), 64, 128, {F32: 64, BF16: 64}),         # M = 105: a partial tile whose rows beyond M must store nothing
    ((4, 64, 32, 32), 128, 256, {F32: 64, BF16: 64}),
    ((8, 64, 32, 32), 256, 256, {F32: 128, BF16: 128}),
    ((4, 64, 64, 64), 256, 256, {F32: 128, BF16: 256}),
]
_KINDS = [(F32, True), (F32, False), (BF16, False)]         # (dtype, integer operands)
_KIND_IDS = ["fp32-int-exact", "fp32-float64", "bf16-float64"]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype,ints", _KINDS, ids=_KIND_IDS)
@pytest.mark.parametrize("shape,cout,rows,cols", _SHAPES)
def test_forward_scatter_elementwise(dev, shape, cout, rows, cols, dtype, ints, bias):
    """insar_igemm mode 1. No variant is forced with a knob; every variant the selector can give for N = 4*Cout is reached
    by one of the shapes (the 128 x 128 tile cannot be: see _SHAPES)."""
    from insar_unet_ca_amd import _lib, engine
    from insar_unet_ca_amd._lib import call
    B, cin, h, w = shape
    M, N = B * h * w, 4 * cout
    assert call("insar_igemm_tile_rows", M, N) == rows
    assert call("insar_igemm_tile_cols_dt", M, N, _lib.dtype_code(dtype)) == cols[dtype]
    ctx = engine.Ctx(dev, dtype)
    xa = _act(_ints(40, -2, 2, *shape) if ints else cf.make_input(shape), dtype, dev)
    p, gw = _weight(ctx, cin, cout, ints, dev)
    bv = None
    if bias:
        bv = (_ints(42, -5, 5, cout).float() if ints else cf.fill_tensor("bias", (cout,), 3)).to(dev)
    cat = engine.Act.alloc(B, 2 * h, 2 * w, 2 * cout, dtype, dev)
    out = cat.slice(cout, cout)
    engine._igemm(xa, out, gw.fwd(), N, h, w, 1, [(0, 0)], 1, bias=bv)
    torch.cuda.synchronize()
    xr, wr = xa.nchw().double(), _w_fwd(gw, cin, cout)
    ref = R.conv_transpose_k2s2(xr, wr, None if bv is None else bv.double())
    got = out.nchw()
    if ints:
        assert float(ref.abs().max()) < 2 ** 24
        assert torch.equal(got.double(), ref), f"{int((got.double() != ref).sum())} of {ref.numel()} elements differ"
    else:
        assert _max_rel(got, ref) <= _out_tol(dtype)
    assert float(cat.slice(0, cout).nchw().abs().max()) == 0.0          # the skip half of the concat buffer untouched
    assert _halo_abs(cat) == 0.0


# The input-gradient GEMM has N = Cin: the forward shapes (Cin 64 or 128) all take 128 x 64 tiles there, so three more with
# the Cin of the U-Net's deep up layers reach the 256-row variants: tile rows, tile columns {dtype}.
_DGRAD_SHAPES = [(shape, cout, 128, {F32: 64, BF16: 64}) for shape, cout, _, _ in _SHAPES] + [
    ((8, 256, 32, 32), 64, 256, {F32: 64, BF16: 64}),          # 32 x 4 tiles of 256 x 64: half the chip
    ((4, 512, 64, 64), 64, 256, {F32: 128, BF16: 128}),
    ((4, 1024, 64, 64), 64, 256, {F32: 128, BF16: 256}),
]


@pytest.mark.parametrize("dtype,ints", _KINDS, ids=_KIND_IDS)
@pytest.mark.parametrize("shape,cout,rows,cols", _DGRAD_SHAPES)
def test_input_gradient_elementwise(dev, shape, cout, rows, cols, dtype, ints):
    """insar_igemm mode 0, stride 2, taps {0,1}^2, no bstat: dx = conv2d(g, w, stride=2) (the identity
    test_wgrad_ref_host.py checks the reference's dx against), on every tile variant the selector gives for N = Cin
    (128 x 128 is unreachable here for the reason given at _SHAPES)."""
    from insar_unet_ca_amd import _lib, engine
    from insar_unet_ca_amd._lib import call
    B, cin, h, w = shape
    assert call("insar_igemm_tile_rows", B * h * w, cin) == rows
    assert call("insar_igemm_tile_cols_dt", B * h * w, cin, _lib.dtype_code(dtype)) == cols[dtype]
    ctx = engine.Ctx(dev, dtype)
    p, gw = _weight(ctx, cin, cout, ints, dev)
    gshape = (B, cout, 2 * h, 2 * w)
    dcat = engine.Act.alloc(B, 2 * h, 2 * w, 2 * cout, dtype, dev)
    engine.pack_input((_ints(43, -2, 2, *gshape).float() if ints else cf.make_grad(gshape)).to(dev), dcat.slice(cout, cout))
    dout = dcat.slice(cout, cout)
    dx = engine.Act.alloc(B, h, w, cin, dtype, dev)
    engine._igemm(dout, dx, gw.dgrad(), cin, h, w, 2, engine._TAPS2, 0)
    torch.cuda.synchronize()
    gr, wr = dout.nchw().double(), _w_dgrad(gw, cin, cout)
    ref = R.conv_transpose_k2s2_backward(torch.zeros((B, cin, h, w), dtype=torch.float64, device=dev), wr, gr)[0]
    got = dx.nchw()
    if ints:
        assert float(ref.abs().max()) < 2 ** 24
        assert torch.equal(got.double(), ref), f"{int((got.double() != ref).sum())} of {ref.numel()} elements differ"
    else:
        assert _max_rel(got, ref) <= _out_tol(dtype)
    assert _halo_abs(dx) == 0.0


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def _plan(dev, dtype, shape, cout, out_hw=None, ints=False):
    from insar_unet_ca_amd import engine
    B, cin, h, w = shape
    H, W = out_hw or (2 * h, 2 * w)
    ctx = engine.Ctx(dev, dtype)
    mod = torch.nn.ConvTranspose2d(cin, cout, 2, 2)
    if ints:
        mod.load_state_dict({"weight": _ints(51, -2, 2, cin, cout, 2, 2).float(), "bias": _ints(52, -5, 5, cout).float()})
    else:
        mod.load_state_dict(cf.fill_state_dict(mod.state_dict()))
    mod = mod.to(dev)
    xa = _act(_ints(50, -2, 2, *shape) if ints else cf.make_input(shape), dtype, dev)
    cat = engine.Act.alloc(B, H, W, 2 * cout, dtype, dev)
    up = engine.UpPlan(ctx, mod, xa, cat.slice(cout, cout), "up")
    dcat = engine.Act.alloc(B, H, W, 2 * cout, dtype, dev)
    gshape = (B, cout, H, W)
    engine.pack_input((_ints(53, -3, 3, *gshape).float() if ints else cf.make_grad(gshape)).to(dev), dcat.slice(cout, cout))
    return ctx, mod, xa, cat, up, dcat


def _backward(ctx, up, dcat, cout, shape, dtype, dev):
    from insar_unet_ca_amd import engine
    B, cin, h, w = shape
    sink = engine.GradSink(ctx, up.params())
    sink.flat().fill_(float("nan"))
    dx = engine.Act.alloc(B, h, w, cin, dtype, dev)
    up.backward(dcat.slice(cout, cout), sink, dx)
    ctx.join_side()
    torch.cuda.synchronize()
    return sink, dx


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape,cout", [((2, 128, 8, 8), 64), ((2, 256, 16, 16), 256), ((3, 64, 5, 7), 64)])
def test_up_plan_against_float64(dev, shape, cout, dtype, monkeypatch):
    """UpPlan.forward and .backward: out, dx, dW (layout 1: (Ci, Co, 2, 2)) and dbias elementwise. 256 -> 256 takes the
    256 x 256 weight-gradient tile in bf16 (128 x 128 with 8 waves in fp32) with the engine's own split factor > 1."""
    from insar_unet_ca_amd import engine
    B, cin, h, w = shape
    seen = []
    launch = engine._launch_wgrad
    monkeypatch.setattr(engine, "_launch_wgrad", lambda d, *a: (seen.append(int(d.nsplit)), launch(d, *a))[1])
    ctx, mod, xa, cat, up, dcat = _plan(dev, dtype, shape, cout)
    up.forward()
    sink, dx = _backward(ctx, up, dcat, cout, shape, dtype, dev)
    assert len(seen) == 1
    if cin == 256:
        assert seen[0] > 1, "the cost model no longer splits this layer: pick a shape where it does"
        assert engine._wgrad_tiles(cin, cout, ctx.code) == ((256, 256) if dtype == BF16 else (128, 128))
    xr, gr = xa.nchw().double(), dcat.slice(cout, cout).nchw().double()
    ref = R.conv_transpose_k2s2(xr, _w_fwd(up.w, cin, cout), mod.bias.detach().double())
    assert _max_rel(cat.slice(cout, cout).nchw(), ref) <= _out_tol(dtype)
    assert float(cat.slice(0, cout).nchw().abs().max()) == 0.0 and _halo_abs(cat) == 0.0
    rdx, rdw, rdb = R.conv_transpose_k2s2_backward(xr, _w_dgrad(up.w, cin, cout), gr)
    assert _max_rel(dx.nchw(), rdx) <= _out_tol(dtype)
    assert _halo_abs(dx) == 0.0
    assert _max_rel(sink.view(mod.weight), rdw) <= KERNEL_TOL * 5
    assert _max_rel(sink.view(mod.bias), rdb) <= KERNEL_TOL * 5


def test_up_plan_integer_operands_are_exact_in_fp32(dev):
    """Integer x, weights, bias and dout in fp32: out, dx, dW and dbias have one right answer each."""
    shape, cout = (3, 64, 5, 7), 64
    B, cin, h, w = shape
    ctx, mod, xa, cat, up, dcat = _plan(dev, F32, shape, cout, ints=True)
    up.forward()
    sink, dx = _backward(ctx, up, dcat, cout, shape, F32, dev)
    xi, gi = xa.nchw().long(), dcat.slice(cout, cout).nchw().long()
    wi, bi = mod.weight.detach().long(), mod.bias.detach().long()
    assert torch.equal(cat.slice(cout, cout).nchw().long(), R.conv_transpose_k2s2(xi, wi, bi))
    rdx, rdw, rdb = R.conv_transpose_k2s2_backward(xi, wi, gi)
    assert torch.equal(dx.nchw().double(), rdx.double())
    assert torch.equal(sink.view(mod.weight).double(), rdw.double())
    assert torch.equal(sink.view(mod.bias).double(), rdb.double())


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_up_plan_with_the_one_pixel_resize(dev, dtype):
    """(2, 64, 6, 7) -> a 12 x 14 conv output resized bilinearly (align_corners=False) into a 13 x 15 skip slice, and the
    adjoint on the way back. `out` is held to the float64 transposed conv followed by the float64 resize; the gradient of
    the conv output to the float64 adjoint of the resize; dx / dW / dbias to float64 on that stored gradient (the kernels'
    own operand), so that every link of the chain is held to float64 of what it was given."""
    shape, cout, out_hw = (2, 64, 6, 7), 64, (13, 15)
    B, cin, h, w = shape
    ctx, mod, xa, cat, up, dcat = _plan(dev, dtype, shape, cout, out_hw=out_hw)
    assert up.resize
    up.forward()
    sink, dx = _backward(ctx, up, dcat, cout, shape, dtype, dev)
    xr, gr = xa.nchw().double().cpu(), dcat.slice(cout, cout).nchw().double().cpu()
    conv = R.conv_transpose_k2s2(xr, _w_fwd(up.w, cin, cout).cpu(), mod.bias.detach().double().cpu()).requires_grad_()
    ref = F.interpolate(conv, size=out_hw, mode="bilinear", align_corners=False)
    ref.backward(gr)
    tol = RESIZE_TOL[dtype]
    assert _max_rel(cat.slice(cout, cout).nchw().cpu(), ref.detach()) <= tol
    assert float(cat.slice(0, cout).nchw().abs().max()) == 0.0 and _halo_abs(cat) == 0.0
    assert _max_rel(up.dconv_out.nchw().cpu(), conv.grad) <= tol
    gconv = up.dconv_out.nchw().double().cpu()
    rdx, rdw, rdb = R.conv_transpose_k2s2_backward(xr, _w_dgrad(up.w, cin, cout).cpu(), gconv)
    assert _max_rel(dx.nchw().cpu(), rdx) <= _out_tol(dtype)
    assert _max_rel(sink.view(mod.weight).cpu(), rdw) <= KERNEL_TOL * 5
    assert _max_rel(sink.view(mod.bias).cpu(), rdb) <= KERNEL_TOL * 5


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_up_plan_gradients_do_not_depend_on_the_issue_order(dev, dtype, monkeypatch):
    """engine.WGRAD_LATE moves the weight-gradient launches behind the input-gradient GEMM: same bits either way."""
    from insar_unet_ca_amd import engine
    shape, cout = (2, 128, 8, 8), 64
    res = []
    for late in (False, True):
        monkeypatch.setattr(engine, "WGRAD_LATE", late)
        ctx, mod, xa, cat, up, dcat = _plan(dev, dtype, shape, cout)
        up.forward()
        sink, dx = _backward(ctx, up, dcat, cout, shape, dtype, dev)
        res.append((dx.buf.clone(), sink.view(mod.weight).clone(), sink.view(mod.bias).clone()))
    for a, b in zip(*res):
        assert not bool(torch.isnan(a.float()).any()) and torch.equal(a, b)
