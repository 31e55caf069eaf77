"""GPU: the pointwise kernels of the ResNet-50 trunk (csrc/deeplab.hip) — the 7x7 stride-2 stem and its weight gradient,
MaxPool2d(3, 2, 1), the residual add, the ReLU gradient gate, the image sums, their broadcast (plain and gated) and dropout —
one launch at a time against the float64 reference tests/pointwise_ref.py.

Conventions and the one tolerance rule are those of tests/test_forward_apply_gpu.py (planted stored operands, ReLU margin,
NaN pre-fill, a sentinel in the halo ring and in the neighbouring channels of a slice, every launch twice and bit for bit
the same; |got - ref| <= K * 2^-24 * U, half a bf16 ulp more for a bf16 store, exact outputs bit for bit). K = 2.76 was fixed
on the CPU before any kernel ran (tests/test_pointwise_ref_host.py):
    largest float32 floor ratio per output (each rounded up to the next 0.01)
        bn_add_relu 0.68  sum_hw 0.45  broadcast_hw 0.77  stem 0.58  stem_stats 1.01  stem_wgrad 0.91
Kernel, measured on an MI355X (largest ratio per output over all cases of this file):
        bn_add_relu 0.66  sum_hw 0.22  broadcast_hw 0.93  stem 0.56  stem_stats 0.83  stem_wgrad 1.01 (folded 0.41)
    nothing needed more than 1.01 of the 2.76 allowed; every exact output matched bit for bit.

Geometry (DL_THREADS = 256; a chunk is 4 fp32 / 8 bf16 channels; every row kernel walks e = w * cpp + cc in steps of 256 and
rows in steps of insar_grid_cap = 8192; the stem: one work-group per output row, 32 pixel lanes x 8 channel groups, so
`wo += 32` makes ceil(Wo / 32) passes; its weight gradient: ST_RPB = 8 consecutive rows (n, ho) per work-group):

  entry point                  path                                                          cases
  insar_conv7x7s2_fwd          Wo = 1, 31, 32, 33, 70 (1..3 passes, idle lanes); Ho = 1, 9      stem: wo1 wo31 wo32 wo33 wo70
                               stats NaN-prefilled, every row written; stats == null         every stem case
                               bf16 inputs not representable (dl_round of x and w)             stem: *-bf16-raw
                               LDS over 160 KiB: W = 4814 refused, nothing launched            stem_too_wide
  insar_conv7x7s2_wgrad        B*Ho = 27 (no multiple of 8), blocks straddling two images      stem: wo1 wo33 (B = 3, Ho = 9)
                               partials per block and folded; W = 1050 refused                 every stem case; stem_too_wide
  insar_maxpool3s2_fwd / _bwd  odd H, odd W, both, 1xW, Hx1; ties at each of the 9 taps, a      pool3: 7x9 8x9 9x8 1x5 5x1 12x20
                               constant channel (clipped windows), NaN, an all -inf channel
  insar_bn_add_relu            relu 0 / 1, C = 64 / 256, slices, B*H = 8200                    bn_add_relu (res never aliases dst in
                                                                                             deeplab.py / fcn.py: not tested aliased)
  insar_relu_gate_bwd          in place / out of place; out = 0, -0.0, smallest positive,     relu_gate_bwd
                               NaN
  insar_sum_hw                 HW 1 63 64 65 1000; C = 64 / 192 (cb > 0); factor != 1;          sum_hw: every SUMHW_CASES id x
                               bf16 -> fp32 and -> bf16                                        (fp32, bf16->fp32, bf16->bf16)
  insar_broadcast_hw / _gate   fp32 src into bf16 dst; accumulate 0 / 1; factor 1 exact;      broadcast
                               gate > 0, == 0, < 0, NaN; the zero overwrites a held value
  insar_dropout                p = 0, 0.5, 1 - 2^-24; slices; mask bytes 0 / 1, the same in    dropout
                               both dtypes; stored mask re-applied; keep count within 6 sigma
  every one                    INSAR_FAIL conditions of the host wrappers                      refusals

No kernel of deeplab.hip had to change. Wall time of the file on an MI355X: 1.5 s for its 108 tests
(the slowest, 0.3 s, is the first launch)."""
import math

import pytest
import torch

from tests import pointwise_cases as PC
from tests import pointwise_ref as R
from tests.pointwise_cases import BF16, F32, F64, tname
from tests.test_bn_backward_chain_gpu import SENTINEL, enforce_margin, interior, nan_buf, outside_untouched, upload
from tests.test_forward_apply_gpu import E_ARG, E_DTYPE, E_SHAPE, K, out_act, refused, twice

pytestmark = pytest.mark.gpu
INF = float("inf")
MEASURED = {}


def check(name, got, ref, unit, bf16_out=False):
    r = R.excess(got.detach().cpu(), ref, unit, K, bf16_out)
    MEASURED[name] = max(MEASURED.get(name, 0.0), r)
    print(f"ratio {name}: {r:.3f}")
    assert r <= K, (name, r)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def guarded(dev, n, fill=float("nan")):
    """A flat fp32 output of n elements with four sentinels behind it."""
    t = torch.full((n + 4,), fill, device=dev)
    t[n:] = SENTINEL
    return t


# ---------------------------------------------------------------------------------------------------------- the stem
STEM = [(n, F32, True) for n in PC.STEM_CASES] + [(n, BF16, r) for n in PC.STEM_CASES for r in (True, False)]


@pytest.mark.parametrize("name,T,rep", STEM, ids=[f"{n}-{tname(T)}{'' if r else '-raw'}" for n, T, r in STEM])
def test_stem(dev, name, T, rep):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    c = PC.stem_case(name, T, rep)
    B, H, W = c["B"], c["H"], c["W"]
    Ho, Wo = H // 2, W // 2
    rows, nb = call("insar_conv7x7s2_fwd_rows", B, H), call("insar_conv7x7s2_wgrad_blocks", B, Ho)
    assert rows == B * Ho and nb == -(-B * Ho // 8)
    x_d, w_d = c["x"].to(dev), c["w"].to(dev)

    def fwd(with_stats=True):
        ya = out_act(dev, (B, Ho, Wo, 64), T, 192, 64)
        st = guarded(dev, rows * 128)
        call("insar_conv7x7s2_fwd", ptr(x_d), H, W, ptr(w_d), ya.ref, ptr(st) if with_stats else 0, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(ya) and bool((st[-4:] == SENTINEL).all())
        return interior(ya), st[:-4].view(rows, 2, 64).cpu()
    y, st = twice(fwd)
    check("stem", y, *R.conv7x7s2(c["x"], c["w"], T), T == BF16)
    check("stem_stats", st, *R.stem_stats(y))                                   # of the STORED y; a row left unwritten is a NaN
    y0, st0 = fwd(False)
    assert R.bits_equal(y0, y) and bool(torch.isnan(st0).all())                 # stats == null: accepted, nothing written
    ga = upload(dev, c["dy"], 192, 64)

    def wgrad():
        part = guarded(dev, nb * 3136)
        call("insar_conv7x7s2_wgrad", ptr(x_d), H, W, ga.ref, ptr(part), stream_ptr())
        torch.cuda.synchronize()
        assert bool((part[-4:] == SENTINEL).all()) and outside_untouched(ga)
        return (part[:-4].view(nb, 3136).cpu(),)
    part, = twice(wgrad)
    ref, u = R.conv7x7s2_wgrad(c["x"], c["dy"], T)
    check("stem_wgrad", part, ref, u)
    check("stem_wgrad_fold", part.double().sum(0), ref.sum(0), u.sum(0))
    assert torch.equal(x_d.cpu(), c["x"]) and torch.equal(w_d.cpu(), c["w"])


@pytest.mark.parametrize("T", [F32, BF16], ids=tname)
def test_stem_too_wide(dev, T):
    """The W at which the staged rows pass 160 KiB of LDS (forward: 7 * (2 Wo + 5) + 7232 floats > 40960 from Wo = 2407;
    weight gradient: 78 Wo + 35 > 40960 from Wo = 525): INSAR_E_SHAPE, nothing launched."""
    from insar_unet_ca_amd._lib import ptr, stream_ptr
    x, w = torch.zeros(2 * 4814, device=dev), torch.zeros(64 * 49, device=dev)
    ya, st = out_act(dev, (1, 1, 2407, 64), T), nan_buf(dev, 128)
    refused(E_SHAPE, "insar_conv7x7s2_fwd", "insar_conv7x7s2_fwd", ptr(x), 2, 4814, ptr(w), ya.ref, ptr(st), stream_ptr())
    ga, part = out_act(dev, (1, 1, 525, 64), T), nan_buf(dev, 3136)
    refused(E_SHAPE, "insar_conv7x7s2_wgrad", "insar_conv7x7s2_wgrad", ptr(x), 2, 1050, ga.ref, ptr(part), stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(interior(ya).float()).all()) and bool(torch.isnan(st).all()) and bool(torch.isnan(part).all())


# ------------------------------------------------------------------------------------------------ insar_maxpool3s2_*
def pool3_input(H, W, T):
    x = PC.rand_act((2, H, W, 64), T, 80 + 10 * H + W)
    x[0, :, :, 0:8] = 0.5                                                       # constant: every window, clipped ones too, ties at its first tap
    if H >= 4 and W >= 4:
        for p in range(9):                                                      # window (1, 1): taps p and 8 equal and largest -> p
            x[0, :, :, 8 + p] = -5.0
            x[0, 1 + p // 3, 1 + p % 3, 8 + p] = 2.0
            x[0, 3, 3, 8 + p] = 2.0
    x[1, :, :, 24:32] = -INF                                                    # -inf everywhere: the first valid tap
    x[1, H // 2, W // 2, 32:40] = float("nan")                                  # one NaN: it wins every window that holds it
    return x


@pytest.mark.parametrize("T", [F32, BF16], ids=tname)
@pytest.mark.parametrize("hw", [(7, 9), (8, 9), (9, 8), (1, 5), (5, 1), (12, 20)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_maxpool3s2(dev, hw, T):
    """Values and arg map exact under the rule (first maximum in scan order inside the image, NaN wins); the backward exact
    against the reference's gather, which tests/test_pointwise_ref_host.py pins to the autograd adjoint."""
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    H, W = hw
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    x = pool3_input(H, W, T)
    xa = upload(dev, x, 192, 64)

    def fwd():
        ya = out_act(dev, (2, Ho, Wo, 64), T, 192, 64)
        arg = torch.full((2 * Ho * Wo * 64 + 16,), 99, dtype=torch.uint8, device=dev)
        call("insar_maxpool3s2_fwd", xa.ref, ya.ref, ptr(arg), stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(ya) and outside_untouched(xa) and bool((arg[-16:] == 99).all())
        return interior(ya), arg[:-16].view(2, Ho, Wo, 64).cpu()
    y, arg = twice(fwd)
    v, a = R.maxpool3s2(x)
    assert R.bits_equal(y, v) and torch.equal(arg, a)
    if H >= 4 and W >= 4:
        assert arg[0, 1, 1, 8:17].tolist() == list(range(9))
    assert int(torch.isnan(y.float()).sum()) > 0 and bool((y[1, :, :, 24:32] == -INF).all())
    dy = PC.rand_act((2, Ho, Wo, 64), T, 81)
    ga, arg_d = upload(dev, dy, 192, 64), arg.to(dev)

    def bwd():
        da = out_act(dev, (2, H, W, 64), T, 192, 64)
        call("insar_maxpool3s2_bwd", ga.ref, ptr(arg_d), da.ref, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(da) and outside_untouched(ga)
        return (interior(da),)
    assert R.bits_equal(twice(bwd)[0], R.maxpool3s2_bwd(dy, arg, H, W, T).to(T))


# ------------------------------------------------------------------------- insar_bn_add_relu, insar_relu_gate_bwd
ADD_SHAPES = {"c64": (2, 3, 7, 64, 1), "c256": (2, 2, 9, 256, 0), "c64-norelu": (1, 2, 65, 64, 0), "rows8200": (2, 4100, 2, 64, 1)}


@pytest.mark.parametrize("name,T", [(n, T) for n in ADD_SHAPES for T in (F32, BF16)], ids=[f"{n}-{t}" for n in ADD_SHAPES for t in PC.DTYPES])
def test_bn_add_relu(dev, name, T):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    B, H, W, Cn, relu = ADD_SHAPES[name]
    c = PC.apply_case((B, H, W, Cn, 0, relu), T, seed=5000 + Cn + H)
    res = PC.rand_act((B, H, W, Cn), T, 90)
    y, _ = enforce_margin(c["y"], c["scale"], c["shift"].double() + res.double(), T)
    sl = (Cn + 128, 64) if H < 100 else (None, 0)
    ya, ra = upload(dev, y, *sl), upload(dev, res, *sl)
    sc, sh = c["scale"].to(dev), c["shift"].to(dev)

    def run():
        da = out_act(dev, (B, H, W, Cn), T, *sl)
        call("insar_bn_add_relu", ya.ref, ptr(sc), ptr(sh), ra.ref, da.ref, relu, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(da) and outside_untouched(ya) and outside_untouched(ra)
        return (interior(da),)
    check("bn_add_relu", twice(run)[0], *R.bn_add_relu(y, c["scale"], c["shift"], res, relu), T == BF16)


@pytest.mark.parametrize("T", [F32, BF16], ids=tname)
def test_relu_gate_bwd(dev, T):
    """g = dout where out > 0: not at 0, -0.0 or NaN, but at the smallest positive value of the dtype (a subnormal). Exact, in
    place (g is dout) and out of place."""
    from insar_unet_ca_amd._lib import call, stream_ptr
    shape = (2, 3, 9, 128)
    out, dout = PC.rand_act(shape, T, 91), PC.rand_act(shape, T, 92)
    tiny = 2.0 ** -133 if T == BF16 else 2.0 ** -149
    for k, v in enumerate((0.0, -0.0, tiny, -tiny, 2.0 ** -126, float("nan"))):
        out[:, :, k, 5::16] = v
    assert float(out[0, 0, 2, 5]) == tiny > 0
    want = R.relu_gate_bwd(dout, out)
    assert bool((want[:, :, 2, 5::16] == dout[:, :, 2, 5::16]).all()) and bool((want[:, :, [0, 1, 3, 5], 5::16] == 0).all())
    oa = upload(dev, out, 256, 64)
    for in_place in (0, 1):
        def run():
            da = upload(dev, dout, 256, 64)
            ga = da if in_place else out_act(dev, shape, T, 256, 64)
            call("insar_relu_gate_bwd", da.ref, oa.ref, ga.ref, stream_ptr())
            torch.cuda.synchronize()
            assert outside_untouched(ga) and outside_untouched(oa) and (in_place or R.bits_equal(interior(da), dout))
            return (interior(ga),)
        assert R.bits_equal(twice(run)[0], want)


# ------------------------------------------------------------------------------ insar_sum_hw, insar_broadcast_hw*
SUM_TYPES = {"fp32": (F32, F32), "bf16-fp32": (BF16, F32), "bf16-bf16": (BF16, BF16)}


@pytest.mark.parametrize("types", list(SUM_TYPES))
@pytest.mark.parametrize("name", list(PC.SUMHW_CASES))
def test_sum_hw(dev, name, types):
    from insar_unet_ca_amd._lib import call, stream_ptr
    T, TO = SUM_TYPES[types]
    B, H, W, Cn, f = PC.SUMHW_CASES[name]
    x = PC.rand_act((B, H, W, Cn), T, 100 + H)
    xa = upload(dev, x, Cn + 128, 64)

    def run():
        oa = out_act(dev, (B, 1, 1, Cn), TO, Cn + 64, 64)
        call("insar_sum_hw", xa.ref, oa.ref, f, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(oa) and outside_untouched(xa)
        return (interior(oa),)
    got, = twice(run)
    ref, u = R.sum_hw(x, f)
    check("sum_hw", got.reshape(B, Cn), ref, u, TO == BF16)


BCAST = [(ts, acc, f, gated) for ts in ("fp32", "fp32-bf16", "bf16-bf16") for acc in (0, 1) for f in (1.0, 0.3) for gated in (0, 1)]


@pytest.mark.parametrize("ts,acc,f,gated", BCAST, ids=[f"{ts}-acc{a}-f{f}-gate{g}" for ts, a, f, g in BCAST])
def test_broadcast_hw(dev, ts, acc, f, gated):
    """dst = (accumulate ? dst : 0) + factor * src[n][c]; with a gate the result is stored as zero where the gate is 0, negative
    or NaN — also where dst held a value. accumulate = 0 with factor 1 and every stored zero are exact."""
    from insar_unet_ca_amd._lib import call, stream_ptr
    TS, T = {"fp32": (F32, F32), "fp32-bf16": (F32, BF16), "bf16-bf16": (BF16, BF16)}[ts]
    B, H, W, Cn = 2, 5, 9, 128
    src, d0 = PC.rand_act((B, 1, 1, Cn), TS, 110), PC.rand_act((B, H, W, Cn), T, 111)
    gate = PC.rand_act((B, H, W, Cn), T, 112)
    gate[:, 0, 0, :], gate[:, 1, 1, :], gate[:, 2, 2, ::2] = 0.0, float("nan"), -0.0
    assert bool((gate > 0).any()) and bool((gate < 0).any())
    sa = upload(dev, src, Cn + 64, 64)
    ga = upload(dev, gate, Cn + 128, 64)

    def run():
        da = upload(dev, d0 if acc else torch.full_like(d0, float("nan")), Cn + 128, 64)
        if gated:
            call("insar_broadcast_hw_gate", sa.ref, da.ref, ga.ref, f, acc, stream_ptr())
        else:
            call("insar_broadcast_hw", sa.ref, da.ref, f, acc, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(da) and outside_untouched(sa) and outside_untouched(ga)
        return (interior(da),)
    got, = twice(run)
    ref, u = R.broadcast_hw(src.reshape(B, Cn), d0, f, acc, gate if gated else None)
    check("broadcast_hw", got, ref, u, T == BF16)
    if gated:
        off = ~(gate.double() > 0)
        assert bool((got[off] == 0).all()) and bool(off[:, 0, 0].all()) and bool(off[:, 1, 1].all())
    if not acc and f == 1.0:                                                    # nothing is computed: the stored src, or +0
        plain = src.to(T).expand(B, H, W, Cn).contiguous()
        assert float(u.max()) == 0.0
        assert R.bits_equal(got, torch.where(gate.double() > 0, plain, torch.zeros(1, dtype=T)) if gated else plain)


# ------------------------------------------------------------------------------------------------------ insar_dropout
P_TOP = 1.0 - 2.0 ** -24       # the largest float below 1: threshold 2^32 - 256, keep probability 2^-24, factor 2^24


@pytest.mark.parametrize("p", [0.0, 0.5, P_TOP], ids=["p0", "p0.5", "p1-2^-24"])
def test_dropout(dev, p):
    """The mask is drawn from (seed, element index of the slice): bytes 0 / 1, the same for both dtypes; out = x / (1 - p) where
    it is set, bit for bit; a stored mask re-applies bit for bit in a second slice (the backward use). Keep count: binomial
    (n, q = 1 - p), sigma = sqrt(n q (1 - q)); |keep - n q| <= ceil(6 sigma): 0 for p = 0, 456 of n = 23040 for p = 0.5, and 1
    for q = 2^-24 (n q = 0.0014)."""
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    shape = (3, 6, 10, 128)
    n, q = 3 * 6 * 10 * 128, 1.0 - p
    masks = {}
    for T in (F32, BF16):
        x = PC.rand_act(shape, T, 120)
        xa = upload(dev, x, 256, 64)

        def run(make=1, given=None):
            da = out_act(dev, shape, T, 256, 128)
            mask = torch.full((n + 16,), 7, dtype=torch.uint8, device=dev)
            if given is not None:
                mask[:n] = given.reshape(-1).to(dev)
            call("insar_dropout", xa.ref, da.ref, ptr(mask), 0 if given is not None else 1234, 0, p, make, stream_ptr())
            torch.cuda.synchronize()
            assert outside_untouched(da) and outside_untouched(xa) and bool((mask[n:] == 7).all())
            return interior(da), mask[:n].view(shape).cpu()
        out, mask = twice(run)
        assert bool((mask <= 1).all())
        assert R.bits_equal(out, R.dropout_apply(x, mask, p, T))
        out2, mask2 = twice(lambda: run(0, mask))
        assert R.bits_equal(out2, out) and torch.equal(mask2, mask)
        keep = int(mask.sum())
        assert abs(keep - n * q) <= math.ceil(6 * math.sqrt(n * q * (1 - q))), keep
        masks[T] = mask
    assert torch.equal(masks[F32], masks[BF16])


# ---------------------------------------------------------------------------------------------------------- refusals
REFUSALS = [
    ("insar_maxpool3s2_fwd", E_SHAPE, lambda x: (x.mk(2, 7, 9, 64).ref, x.mk(2, 3, 5, 64).ref, x.v, x.s)),
    ("insar_maxpool3s2_fwd", E_SHAPE, lambda x: (x.mk(2, 8, 8, 64).ref, x.mk(2, 4, 4, 64, BF16).ref, x.v, x.s)),
    ("insar_maxpool3s2_fwd", E_ARG, lambda x: (x.mk(2, 8, 8, 64).ref, x.mk(2, 4, 4, 64).ref, 0, x.s)),
    ("insar_maxpool3s2_bwd", E_SHAPE, lambda x: (x.mk(2, 4, 4, 64).ref, x.v, x.mk(2, 9, 8, 64).ref, x.s)),
    ("insar_maxpool3s2_bwd", E_ARG, lambda x: (x.mk(2, 4, 4, 64).ref, 0, x.mk(2, 8, 8, 64).ref, x.s)),
    ("insar_bn_add_relu", E_SHAPE, lambda x: (x.y.ref, x.v, x.v, x.mk(2, 4, 5, 64).ref, x.d.ref, 1, x.s)),
    ("insar_bn_add_relu", E_ARG, lambda x: (x.y.ref, x.v, 0, x.d.ref, x.d.ref, 1, x.s)),
    ("insar_bn_add_relu", E_ARG, lambda x: (x.y.ref, x.v, x.v, None, x.d.ref, 1, x.s)),
    ("insar_relu_gate_bwd", E_SHAPE, lambda x: (x.y.ref, x.mk(2, 4, 6, 128).ref, x.d.ref, x.s)),
    ("insar_relu_gate_bwd", E_ARG, lambda x: (x.y.ref, x.d.ref, None, x.s)),
    ("insar_sum_hw", E_SHAPE, lambda x: (x.mk(2, 4, 6, 32).ref, x.mk(2, 1, 1, 32).ref, 1.0, x.s)),
    ("insar_sum_hw", E_SHAPE, lambda x: (x.y.ref, x.mk(2, 1, 2, 64).ref, 1.0, x.s)),
    ("insar_sum_hw", E_DTYPE, lambda x: (x.y.ref, x.mk(2, 1, 1, 64, BF16).ref, 1.0, x.s)),
    ("insar_broadcast_hw", E_DTYPE, lambda x: (x.mk(2, 1, 1, 64, BF16).ref, x.d.ref, 1.0, 0, x.s)),
    ("insar_broadcast_hw", E_SHAPE, lambda x: (x.mk(2, 1, 1, 128).ref, x.d.ref, 1.0, 0, x.s)),
    ("insar_broadcast_hw_gate", E_ARG, lambda x: (x.mk(2, 1, 1, 64).ref, x.d.ref, None, 1.0, 0, x.s)),
    ("insar_broadcast_hw_gate", E_SHAPE, lambda x: (x.mk(2, 1, 1, 64).ref, x.d.ref, x.mk(2, 4, 6, 64, BF16).ref, 1.0, 0, x.s)),
    ("insar_dropout", E_ARG, lambda x: (x.y.ref, x.d.ref, x.v, 1, 0, 1.0, 1, x.s)),
    ("insar_dropout", E_ARG, lambda x: (x.y.ref, x.d.ref, x.v, 1, 0, -0.1, 1, x.s)),
    ("insar_dropout", E_ARG, lambda x: (x.y.ref, x.d.ref, 0, 1, 0, 0.5, 1, x.s)),
    ("insar_dropout", E_SHAPE, lambda x: (x.y.ref, x.mk(2, 4, 5, 64).ref, x.v, 1, 0, 0.5, 1, x.s)),
    ("insar_conv7x7s2_fwd", E_SHAPE, lambda x: (x.v, 7, 12, x.v, x.mk(2, 3, 6, 64).ref, x.ptr(x.lg), x.s)),
    ("insar_conv7x7s2_fwd", E_SHAPE, lambda x: (x.v, 8, 12, x.v, x.mk(2, 4, 6, 128).ref, x.ptr(x.lg), x.s)),
    ("insar_conv7x7s2_fwd", E_ARG, lambda x: (0, 8, 12, x.v, x.y.ref, x.ptr(x.lg), x.s)),
    ("insar_conv7x7s2_wgrad", E_SHAPE, lambda x: (x.v, 8, 10, x.y.ref, x.ptr(x.lg), x.s)),
    ("insar_conv7x7s2_wgrad", E_ARG, lambda x: (x.v, 8, 12, x.y.ref, 0, x.s)),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)), ids=[f"{r[0]}-{i}" for i, r in enumerate(REFUSALS)])
def test_refusals(dev, i):
    """One INSAR_FAIL condition of a host wrapper: the documented code, insar_last_error names the entry point (the gated
    broadcast reports shape and dtype faults of src / dst under insar_broadcast_hw), every output keeps its pre-fill."""
    from tests.test_forward_apply_gpu import RefusalFixture
    name, code, build = REFUSALS[i]
    x = RefusalFixture(dev)
    refused(code, "insar_broadcast_hw" if "broadcast" in name else name, name, *build(x))
    assert x.untouched()


def test_print_measured():
    """Last in the file: the largest kernel ratio per output (visible with -s)."""
    print("MEASURED", "  ".join(f"{k} {v:.2f}" for k, v in sorted(MEASURED.items())))
