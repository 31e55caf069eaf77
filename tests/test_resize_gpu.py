"""GPU: the two bilinear resizes — insar_resize_bilinear_fwd / _bwd (padded NHWC slices, both dtypes, csrc/pointwise.hip) and
insar_bilinear_fwd / _bwd (NCHW fp32 planes, csrc/deeplab.hip) — one launch at a time against the float64 reference
tests/pointwise_ref.resize_fwd / resize_bwd (the adjoint is the explicit transpose of the forward's weights).

Conventions are those of tests/test_forward_apply_gpu.py: stored operands, the destination NaN inside and a sentinel in its halo
ring and in the neighbouring channels of a slice (sources likewise), every launch twice and bit for bit the same, and the rule
|got - ref| <= K * 2^-24 * U (half a bf16 ulp more for a bf16 store) with U = sum |w * x| over an output's four taps and
sqrt(n) * sum |w * g| over an adjoint element's n taps. K = PC.RESIZE_K = 221.04 is twice the float32 floor measured on the CPU
(tests/test_pointwise_ref_host.py): a float32 src moves a tap's weight by about 2^-24 * src. Equal sizes are the identity and
are held bit for bit.

  case (tests/pointwise_cases.RESIZE_CASES)     edge
  up8, up12x20, up-ragged                       2x and ragged up-sampling; 13 <- 5 has an output whose float32 src rounds to the
                                                other side of an integer (o = 6): the neighbouring index pair, weight ~ 2^-23
  down-ragged, down8                            scale above 1: the adjoint's window comes from float divisions
  same                                          the identity, forward and adjoint, bit for bit
  src1x1, src1xW, srcHx1, dst1x1                every clamp of i0 / i1 at once; one output gathering a whole map's adjoint
  plus1, plus1w                                 the U-Net decoder's one-pixel resizes
  NHWC only: C = 64 plain and as a slice [64, 128) of 192 channels on both sides; rows12300 (B * H = 12300 on both sides, above
  the grid cap of 8192; exact power-of-two scale in H); a C that is no multiple of the chunk and a dtype mismatch are refused
  NCHW only: a guard plane of sentinels behind the output

Kernel, measured on an MI355X (largest ratio over the cases; allowed 221.04): see DESIGN.md, "Testing the out-of-bounds
implicit GEMM and the bilinear resizes"."""
import pytest
import torch

from tests import pointwise_cases as PC
from tests import pointwise_ref as R
from tests.pointwise_cases import BF16, F32, tname
from tests.test_bn_backward_chain_gpu import SENTINEL, interior, outside_untouched, upload
from tests.test_forward_apply_gpu import E_SHAPE, out_act, refused, twice

pytestmark = pytest.mark.gpu
K = PC.RESIZE_K
MEASURED = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def check(name, got, ref, unit, bf16_out=False):
    r = R.excess(got.detach().cpu(), ref, unit, K, bf16_out)
    MEASURED[name] = max(MEASURED.get(name, 0.0), r)
    print(f"ratio {name}: {r:.3f}")
    assert r <= K, (name, r)


def _nhwc_pair(dev, x, g, T, ctot, c_off, name):
    """Forward of x and adjoint of g through the NHWC entry points; returns nothing, asserts everything."""
    from insar_unet_ca_amd._lib import call, stream_ptr
    B, hi, wi, cn = x.shape
    ho, wo = g.shape[1:3]
    xa, ga = upload(dev, x, ctot, c_off), upload(dev, g, ctot, c_off)

    def fwd():
        ya = out_act(dev, (B, ho, wo, cn), T, ctot, c_off)
        call("insar_resize_bilinear_fwd", xa.ref, ya.ref, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(ya) and outside_untouched(xa) and R.bits_equal(interior(xa), x)
        return (interior(ya),)

    def bwd():
        dxa = out_act(dev, (B, hi, wi, cn), T, ctot, c_off)
        call("insar_resize_bilinear_bwd", ga.ref, dxa.ref, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(dxa) and outside_untouched(ga) and R.bits_equal(interior(ga), g)
        return (interior(dxa),)
    y, = twice(fwd)
    dx, = twice(bwd)
    if (hi, wi) == (ho, wo):
        assert R.bits_equal(y, x) and R.bits_equal(dx, g), name + ": equal sizes are the identity"
    check(f"resize_fwd {name}", y, *R.resize_fwd(x, (ho, wo)), T == BF16)
    check(f"resize_bwd {name}", dx, *R.resize_bwd(g, (hi, wi)), T == BF16)


NHWC = [(n, T, s) for n in PC.RESIZE_CASES for T in (F32, BF16) for s in (False, True)]


@pytest.mark.parametrize("name,T,sliced", NHWC, ids=[f"{n}-{tname(T)}{'-slice' if s else ''}" for n, T, s in NHWC])
def test_nhwc_resize(dev, name, T, sliced):
    c = PC.resize_case(name, T)
    _nhwc_pair(dev, c["x"], c["g"], T, *((192, 64) if sliced else (None, 0)), name)


@pytest.mark.parametrize("T", [F32, BF16], ids=tname)
def test_nhwc_resize_more_rows_than_the_grid(dev, T):
    """B * H = 12300 source rows and 24600 destination rows: both kernels walk rows in steps of the grid cap (8192). 4100 -> 8200
    has the scale 1/2, exact in float32, so the long axis adds nothing to the floor; 2 -> 3 columns are ragged."""
    g = PC.gen(77)
    draw = lambda *s: ((torch.randint(0, 2, s, generator=g).float() * 2 - 1) * (0.5 + torch.rand(s, generator=g))).to(T)
    _nhwc_pair(dev, draw(3, 4100, 2, 8), draw(3, 8200, 3, 8), T, None, 0, "rows12300")


@pytest.mark.parametrize("name", list(PC.RESIZE_CASES))
def test_nchw_resize(dev, name):
    """insar_bilinear_fwd / _bwd on B * C fp32 planes: NaN-prefilled outputs with a guard plane of sentinels behind them."""
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    c = PC.resize_case(name, F32, Cn=3)
    (hi, wi), (ho, wo) = c["in"], c["out"]
    planes = 2 * 3
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    x_d, g_d = nchw(c["x"]).to(dev), nchw(c["g"]).to(dev)

    def run(entry, src, h, w):
        def go():
            out = torch.full((planes + 1, h, w), float("nan"), device=dev)
            out[planes] = SENTINEL
            call(entry, ptr(src), ptr(out), planes, hi, wi, ho, wo, stream_ptr())
            torch.cuda.synchronize()
            assert bool((out[planes] == SENTINEL).all()), entry + ": wrote behind its output"
            return (out[:planes].reshape(2, 3, h, w).permute(0, 2, 3, 1).cpu(),)
        return twice(go)[0]
    y, dx = run("insar_bilinear_fwd", x_d, ho, wo), run("insar_bilinear_bwd", g_d, hi, wi)
    assert torch.equal(x_d.cpu(), nchw(c["x"])) and torch.equal(g_d.cpu(), nchw(c["g"]))
    if c["in"] == c["out"]:
        assert R.bits_equal(y.contiguous(), c["x"]) and R.bits_equal(dx.contiguous(), c["g"])
    check(f"bilinear_fwd {name}", y, *R.resize_fwd(c["x"], c["out"]))
    check(f"bilinear_bwd {name}", dx, *R.resize_bwd(c["g"], c["in"]))


@pytest.mark.parametrize("entry", ["insar_resize_bilinear_fwd", "insar_resize_bilinear_bwd"])
def test_nhwc_resize_refusals(dev, entry):
    """A channel count that is no multiple of the chunk (4 fp32 / 8 bf16 channels) and a dtype mismatch: refused on the host,
    nothing written."""
    from insar_unet_ca_amd._lib import stream_ptr
    for Ta, Tb, cn in ((F32, F32, 6), (BF16, BF16, 12), (F32, BF16, 64), (BF16, F32, 64)):
        a = upload(dev, torch.ones(2, 4, 5, cn, dtype=Ta))
        b = out_act(dev, (2, 6, 7, cn), Tb)
        refused(E_SHAPE, entry, entry, a.ref, b.ref, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(b) and bool(torch.isnan(interior(b)).all()) and bool((interior(a) == 1).all())


def test_print_measured():
    """Not a check: the largest ratio per entry point, for DESIGN.md (run with -s)."""
    for kind in ("resize_fwd", "resize_bwd", "bilinear_fwd", "bilinear_bwd"):
        vals = {k: v for k, v in MEASURED.items() if k.startswith(kind)}
        if vals:
            worst = max(vals, key=vals.get)
            print(f"largest ratio {kind}: {vals[worst]:.2f} ({worst}); every case: " + "  ".join(f"{k.split()[-1]} {v:.2f}" for k, v in vals.items()))
