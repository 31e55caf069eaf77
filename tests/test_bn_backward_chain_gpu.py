"""GPU: every C-ABI entry point of the [BatchNorm -> ReLU -> (SE gate)] backward chain, insar_bn_finalize and the SE forward
(csrc/pointwise.hip) against the float64 reference tests/bn_chain_ref.py, at unit level.

Each launch is judged on the values it actually read (the stored, dtype-rounded tensors; for a coefficient kernel the
slab the reduce kernel wrote), so an error cannot hide behind the one before it. Shapes are the smallest that reach each
code path (the table at SHAPES). Inputs: seeded noise plus a per-channel offset, |mean| / sigma in {0, 3, 30} across the
channels; every pre-activation closer to 0 than 1e-3 of the tensor's maximum is moved out to that margin before upload
(asserted on the stored values in make_case), so the fp32 kernel and the float64 reference take the same ReLU decision
everywhere and no element is excluded from any comparison. Outputs are pre-filled with NaN, buffers with a sentinel.

Tolerance (one rule, bn_chain_ref's docstring): |got - ref| <= K * 2^-24 * U, U = the reference's running error unit of that
output (sqrt(n) * sum|terms| per sum, propagated through the chain inside one launch, cancelling differences by their
operands' magnitudes); bf16 dy may be half a bf16 ulp of the reference further off. K was fixed BEFORE any kernel ran:
the reference's formulas evaluated in float32 on the CPU in naive order (dt=torch.float32) on these same cases, measured
against float64 (floor_ratios below, all cases of CHAIN_CASES / ROWS_PER_IMAGE / finalize):
    largest float32 floor ratio per output
        reduce 0.93  squeeze 0.89  pooled 0.97  sq 0.79  hid 0.06  gate 0.05  coefB 0.09  dW1 0.08  dW2 0.78
        tb 1.15  tg 0.78  dbeta 0.65  dgamma 0.45  k1 0.47  k2 0.39  dconv_bias 0.53  dy 1.625  dy (from tb / tg) 1.59
        finalize: mean 1.00  invstd 0.83  scale 0.73  shift 0.64  running_mean 0.99  running_var 1.14
    K = 2 * 1.625 = 3.25
Kernel, measured on an MI355X (largest ratio per output over all cases of this file):
        reduce 0.93  reduce_pool 0.81  reduce_outc 0.37  wpart 0.27  squeeze 0.88  pooled 0.90  sq 1.10  hid 0.07  gate 0.05
        coefB 0.09  dW1 0.32  dW2 0.75  tb 1.15  tg 0.70  dbeta 0.61  dgamma 0.57  k1 0.63  k2 0.48  dconv_bias 0.52
        dy 1.01  dy (from tb / tg) 0.94  dy_pool 0.90  dy_outc 0.58
        finalize: mean 0.94  invstd 0.78  scale 0.72  shift 0.64  running_mean 1.12  running_var 1.17
    every entry point of a family (insar_bnse_bwd_coef, _coef_stage, _coef_fused, insar_bn_bwd_coef) gave the same figure to
    two digits; nothing needed more than 1.17 of the 3.25 allowed, the |mean| / sigma = 30 channels included.
"""
import ctypes as C
import math

import pytest
import torch

from tests import bn_chain_ref as R

pytestmark = pytest.mark.gpu

K = 3.25
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SENTINEL = 77.0
MEASURED = {}        # output name -> largest ratio seen (printed per case: run with -s to collect)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------------------- inputs (CPU only)
def enforce_margin(y, scale, shift, T):
    """Move every element whose pre-activation |y*scale + shift| is below 1e-3 of the tensor's maximum out to that margin
    (keeping its sign); returns the stored tensor and the margin, asserted on the stored values."""
    y = y.to(T)
    sc, sh = scale.double(), shift.double()
    a = y.double() * sc + sh
    margin = 1e-3 * float(a.abs().max())
    sgn = torch.where(a >= 0, 1.0, -1.0).double()
    for i in range(1, 40):
        bad = (y.double() * sc + sh).abs() < margin
        if not bool(bad.any()):
            break
        target = ((sgn * (1.0 + i * i) * margin - sh) / sc).to(T)      # further out each round: the dtype's grid is coarse
        y = torch.where(bad, target, y)
    assert float((y.double() * sc + sh).abs().min()) >= margin > 0
    return y, margin


def make_case(B, H, W, Cn, T, seed, Cr=None, lattice=False):
    """Stored tensors of one unit: y, dout (dtype T, NHWC), the BatchNorm constants (fp32) and the SE weights."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    c = {"B": B, "H": H, "W": W, "C": Cn, "T": T, "Cr": Cr or max(1, Cn // 16)}
    sigma = 0.5 + 1.5 * torch.rand(Cn, generator=g, dtype=F64)
    off = torch.tensor([0.0, 3.0, 30.0], dtype=F64)[torch.arange(Cn) % 3] * sigma * torch.where(torch.arange(Cn) % 2 == 0, 1.0, -1.0)
    y = rn(B, H, W, Cn) * sigma + off
    gamma = (0.5 + torch.rand(Cn, generator=g, dtype=F64)) * torch.where(torch.rand(Cn, generator=g) < 0.25, -1.0, 1.0)
    beta = 0.3 * rn(Cn)
    if lattice:          # values on a coarse binary grid: round_T(sum_k dl*W) and round_T(relu(y*scale+shift)*gate) are exact
        y = torch.round(y * 8) / 8
        y = torch.where(y.abs() < 0.125, torch.full_like(y, 0.125), y)
        invstd = torch.exp2(torch.round(torch.log2(1 / sigma)))
        scale = torch.exp2(torch.round(torch.log2(gamma.abs()))) * gamma.sign() * invstd
        mean = torch.round(off * 8) / 8
        shift = torch.round((beta - mean * scale) * 8) / 8
    else:
        yt = y.to(T).double()
        mean = yt.mean((0, 1, 2))
        invstd = 1 / torch.sqrt(yt.var((0, 1, 2), unbiased=False) + 1e-5)
        scale = gamma * invstd
        shift = beta - mean * scale
    c["mean"], c["invstd"], c["scale"], c["shift"] = (t.to(F32) for t in (mean, invstd, scale, shift))
    c["y"], c["margin"] = enforce_margin(y, c["scale"], c["shift"], T)
    c["dout"] = (rn(B, H, W, Cn) * (0.5 + torch.rand(Cn, generator=g, dtype=F64))).to(T)
    c["w1"] = (rn(c["Cr"], Cn) / math.sqrt(Cn)).to(F32)
    c["w2"] = (rn(Cn, c["Cr"]) * 2 / math.sqrt(c["Cr"])).to(F32)
    return c


def synthetic_se(B, Cn, Cr, HW, seed):
    """Stored SE forward results for a coefficient kernel fed a synthetic slab: any values of the right kind will do."""
    g = torch.Generator().manual_seed(seed)
    cnt = torch.randint(0, HW + 1, (B, Cn), generator=g).float()
    pooled = torch.stack([cnt, cnt * torch.randn(B, Cn, generator=g)], 1)
    hid = torch.randn(B, Cr, generator=g).clamp_min(0)
    return dict(pooled=pooled, sq=torch.randn(B, Cn, generator=g), hid=hid, gate=torch.sigmoid(torch.randn(B, Cn, generator=g)))


def synthetic_slab(B, rows, Cn, seed):
    g = torch.Generator().manual_seed(seed)
    red = torch.randn(B, rows, 2, Cn, generator=g) + 0.5 * torch.randn(1, 1, 2, Cn, generator=g)
    sigma = 0.5 + torch.rand(Cn, generator=g)
    mean = torch.tensor([0.0, 3.0, 30.0])[torch.arange(Cn) % 3] * sigma
    red[:, :, 1] = red[:, :, 1] * sigma + red[:, :, 0] * mean          # Q = sum g*mask*y with y = mean + sigma*noise
    invstd = 1 / sigma
    scale = invstd * (0.5 + torch.rand(Cn, generator=g)) * torch.where(torch.arange(Cn) % 5 == 0, -1.0, 1.0)
    return red.float(), dict(mean=mean.float(), invstd=invstd.float(), scale=scale.float(),
                             shift=(0.3 * torch.randn(Cn, generator=g) - mean * scale).float())


def floor_ratios(c, relu, training, use_se, rpp):
    """The float32-in-naive-order floor of one case against float64, per output: {name: ratio} (CPU only; fixes K)."""
    out = {}
    cs = (c["scale"], c["shift"])
    for name, dout in (("reduce", c["dout"]), ("squeeze", None)):
        ref, u = R.reduce(dout, c["y"], *cs, relu, rpp)
        lo, _ = R.reduce(dout, c["y"], *cs, relu, rpp, dt=F32)
        out[name] = R.ratio(lo, ref, u)
    red = R.reduce(c["dout"], c["y"], *cs, relu, rpp)[0].float()
    se = {}
    if use_se:
        sp = R.reduce(None, c["y"], *cs, relu, rpp)[0].float()
        ref, u = R.se_forward(c["y"], *cs, c["w1"], c["w2"], relu, part=sp)
        lo, _ = R.se_forward(c["y"], *cs, c["w1"], c["w2"], relu, part=sp, dt=F32)
        for k in ref:
            out[k] = R.ratio(lo[k], ref[k], u[k])
        se = {k: v.float() for k, v in ref.items()}
        se.update(w1=c["w1"], w2=c["w2"])
    args = (red, c["H"], c["W"], *cs, c["mean"], c["invstd"], training, use_se)
    ref, u = R.coef(*args, **se)
    lo, _ = R.coef(*args, **se, dt=F32)
    for k in ref:
        out[k] = R.ratio(lo[k], ref[k], u[k])
    st = {k: v.float() for k, v in ref.items()}
    for name, kk in (("dy", dict(k1=st["k1"], k2=st["k2"])), ("dy_part", dict(tb=st["tb"], tg=st["tg"]))):
        a = (c["dout"], c["y"], *cs, c["mean"], c["invstd"], relu, se.get("gate"), st.get("coefB"))
        ref, u = R.apply(*a, **kk)
        lo, _ = R.apply(*a, **kk, dt=F32)
        out[name] = R.ratio(lo, ref, u)
    return out


# --------------------------------------------------------------------------------------------------- device helpers
def upload(dev, t, Ctot=None, c_off=0):
    """NHWC tensor -> Act slice [c_off, c_off + C) of a padded buffer whose every other byte holds a sentinel."""
    from insar_unet_ca_amd import engine
    B, H, W, Cn = t.shape
    a = engine.Act.alloc(B, H, W, Ctot or Cn, t.dtype, dev)
    a.buf.fill_(SENTINEL)
    a = a.slice(c_off, Cn) if Ctot else a
    a.buf[:, 1:-1, 1:-1, a.c_off:a.c_off + Cn] = t.to(dev)
    return a


def interior(a):
    return a.buf[:, 1:-1, 1:-1, a.c_off:a.c_off + a.c_len].cpu()


def outside_untouched(a):
    """Every byte outside the slice's interior still holds the sentinel."""
    b = a.buf.clone()
    b[:, 1:-1, 1:-1, a.c_off:a.c_off + a.c_len] = SENTINEL
    return bool((b == SENTINEL).all())


def nan_buf(dev, *shape):
    return torch.full(shape, float("nan"), dtype=F32, device=dev)


def check(name, got, ref, unit, half_ulp_bf16=False):
    got, ref = got.detach().cpu().double().reshape(ref.shape), ref.double()
    unit = torch.as_tensor(unit, dtype=F64).expand_as(ref)
    if half_ulp_bf16:
        assert bool(torch.isfinite(got).all()), name
        slack = R.bf16_half_ulp(ref, K * R.EPS32 * unit)
        r = R.ratio(((got - ref).abs() - slack).clamp_min(0), torch.zeros_like(ref), unit)
    else:
        r = R.ratio(got, ref, unit)
    MEASURED[name] = max(MEASURED.get(name, 0.0), r)
    print(f"ratio {name}: {r:.3f}")
    assert r <= K, (name, r)


def devs(dev, c, *names):
    return [c[n].to(dev) for n in names]


def run_reduce(dev, c, ya, ga, relu, rpp):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    P = -(-c["H"] // rpp)
    sc, sh = devs(dev, c, "scale", "shift")
    part = nan_buf(dev, c["B"], P, 2, c["C"])
    call("insar_bnrelu_bwd_reduce", ga.ref, ya.ref, ptr(sc), ptr(sh), ptr(part), relu, rpp, stream_ptr())
    torch.cuda.synchronize()
    check("reduce", part, *R.reduce(interior(ga), interior(ya), c["scale"], c["shift"], relu, rpp))
    return part


def run_se_forward(dev, c, ya, relu, rpp):
    from insar_unet_ca_amd._lib import InsarSeFwd, call, ptr, stream_ptr
    B, H, W, Cn, Cr = c["B"], c["H"], c["W"], c["C"], c["Cr"]
    P = -(-H // rpp)
    sc, sh, w1, w2 = devs(dev, c, "scale", "shift", "w1", "w2")
    spart = nan_buf(dev, B, P, 2, Cn)
    call("insar_se_squeeze", ya.ref, ptr(sc), ptr(sh), ptr(spart), relu, rpp, stream_ptr())
    torch.cuda.synchronize()
    check("squeeze", spart, *R.reduce(None, interior(ya), c["scale"], c["shift"], relu, rpp))
    out = dict(pooled=nan_buf(dev, B, 2, Cn), sq=nan_buf(dev, B, Cn), hid=nan_buf(dev, B, Cr), gate=nan_buf(dev, B, Cn))
    d = InsarSeFwd()
    d.part, d.rows, d.B, d.H, d.W, d.C, d.Cr = ptr(spart), P, B, H, W, Cn, Cr
    d.scale, d.shift, d.w1, d.w2 = ptr(sc), ptr(sh), ptr(w1), ptr(w2)
    d.pooled, d.sq, d.hid, d.gate = (ptr(out[k]) for k in ("pooled", "sq", "hid", "gate"))
    call("insar_se_excite", C.byref(d), stream_ptr())
    torch.cuda.synchronize()
    ref, u = R.se_forward(interior(ya), c["scale"], c["shift"], c["w1"], c["w2"], relu, part=spart.cpu())
    for k in ref:
        check(k, out[k], ref[k], u[k])
    return {k: v.cpu() for k, v in out.items()}


def run_coef(dev, red, H, W, bn, training, accumulate, se=None, w=None, variants=("coef", "stage", "fused", "fused2", "bn"),
             seed=0):
    """Every coefficient entry point on the same slab red[B][rows][2][C] (a device tensor), each against float64. Returns
    the stored results of the first variant and the stage-1 scratch (tb, tg)."""
    from insar_unet_ca_amd._lib import InsarBnSeBwd, InsarError, call, ptr, stream_ptr
    B, rows, _, Cn = red.shape
    use_se = int(se is not None)
    Cr = w[0].shape[0] if use_se else 1
    sc, sh, mu, istd = (bn[k].to(dev) for k in ("scale", "shift", "mean", "invstd"))
    sed = {k: v.to(dev) for k, v in (se or {}).items()}
    wd = [t.to(dev) for t in (w or ())]
    ref, u = R.coef(red.cpu(), H, W, bn["scale"], bn["shift"], bn["mean"], bn["invstd"], training, use_se,
                    **(dict(se, w1=w[0], w2=w[1]) if use_se else {}))
    g = torch.Generator().manual_seed(100 + seed)
    acc_names = ["dgamma", "dbeta", "dconv_bias"] + (["dW1", "dW2"] if use_se else [])
    init = {k: torch.randn(ref[k].shape, generator=g).float() for k in acc_names}
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    first, parts = None, None
    for v in variants:
        if v == "bn" and use_se:
            continue
        o = {k: (init[k].to(dev) if accumulate else nan_buf(dev, *ref[k].shape)) for k in acc_names}
        o.update(k1=nan_buf(dev, Cn), k2=nan_buf(dev, Cn), coefB=nan_buf(dev, B, Cn))
        ws = nan_buf(dev, B * (3 * Cn + Cr))
        d = InsarBnSeBwd()
        d.B, d.H, d.W, d.C, d.Cr, d.use_se, d.accumulate = B, H, W, Cn, Cr, use_se, accumulate
        d.mean, d.invstd, d.dgamma, d.dbeta, d.k1, d.k2 = ptr(mu), ptr(istd), ptr(o["dgamma"]), ptr(o["dbeta"]), ptr(o["k1"]), ptr(o["k2"])
        if use_se:
            d.pooled, d.sq, d.hid, d.gate = (ptr(sed[k]) for k in ("pooled", "sq", "hid", "gate"))
            d.w1, d.w2, d.dw1, d.dw2, d.coefB = ptr(wd[0]), ptr(wd[1]), ptr(o["dW1"]), ptr(o["dW2"]), ptr(o["coefB"])
        args = (C.byref(d), ptr(red), rows, ptr(sc), ptr(sh), ptr(ws), ptr(o["dconv_bias"]), training)
        s = stream_ptr()
        if v == "coef":
            call("insar_bnse_bwd_coef", *args, s)
        elif v == "stage":
            call("insar_bnse_bwd_coef_stage", *args, 1, s)
            torch.cuda.synchronize()
            assert bool(torch.isnan(o["k1"]).all())                       # stage 1 alone leaves the batch fold alone
            call("insar_bnse_bwd_coef_stage", *args, 2, s)
        elif v in ("fused", "fused2"):                                   # twice through one ticket: it resets itself
            call("insar_bnse_bwd_coef_fused", *args, ptr(ticket), s)
        else:
            call("insar_bn_bwd_coef", C.byref(d), ptr(red), B * rows, ptr(sc), ptr(o["dconv_bias"]), training, s)
        torch.cuda.synchronize()
        assert int(ticket) == 0
        for k in ["dgamma", "dbeta", "k1", "k2", "dconv_bias"] + (["coefB", "dW1", "dW2"] if use_se else []):
            r_, u_ = ref[k], u[k]
            if accumulate and k in init:
                r_, u_ = r_ + init[k].double(), u_ + init[k].double().abs() + ref[k].abs()
            check(f"{k}[{v}]", o[k], r_, u_)
        if v != "bn":
            tb = ws[B * (Cn + Cr):].view(2, B, Cn)
            check(f"tb[{v}]", tb[0], ref["tb"], u["tb"])
            check(f"tg[{v}]", tb[1], ref["tg"], u["tg"])
            parts = parts or (ws, tb)
        first = first or {k: t.cpu() for k, t in o.items()}
    return first, parts


def run_apply(dev, c, ya, ga, relu, coefs, parts, se, dy_slice=None):
    from insar_unet_ca_amd._lib import InsarError, call, ptr, stream_ptr
    T, Cn = c["T"], c["C"]
    sc, sh, mu, istd = devs(dev, c, "scale", "shift", "mean", "invstd")
    gate = se["gate"].to(dev) if se else None
    coefB = coefs["coefB"].to(dev) if se else None
    k1, k2 = coefs["k1"].to(dev), coefs["k2"].to(dev)
    zeros = torch.zeros(c["B"], c["H"], c["W"], Cn, dtype=T)
    bn = (c["scale"], c["shift"], c["mean"], c["invstd"], relu, se["gate"] if se else None, coefs["coefB"] if se else None)
    dya = upload(dev, zeros, *(dy_slice or ()))
    call("insar_bnrelu_bwd_apply", ga.ref, ya.ref, ptr(sc), ptr(sh), ptr(mu), ptr(istd), ptr(gate), ptr(coefB), ptr(k1), ptr(k2),
         dya.ref, relu, stream_ptr())
    torch.cuda.synchronize()
    check("dy", interior(dya), *R.apply(interior(ga), interior(ya), *bn, k1=coefs["k1"], k2=coefs["k2"]), half_ulp_bf16=T == BF16)
    assert outside_untouched(dya) and outside_untouched(ya) and outside_untouched(ga)
    if parts is None:
        return
    tb = parts[1]
    dyp = upload(dev, zeros, *(dy_slice or ()))
    pargs = (ga.ref, ya.ref, ptr(sc), ptr(sh), ptr(mu), ptr(istd), ptr(gate), ptr(coefB), tb[0].data_ptr(), tb[1].data_ptr(), dyp.ref,
             relu, stream_ptr())
    if Cn > 1024:
        with pytest.raises(InsarError):
            call("insar_bnrelu_bwd_apply_part", *pargs)
        return
    call("insar_bnrelu_bwd_apply_part", *pargs)
    torch.cuda.synchronize()
    check("dy_part", interior(dyp), *R.apply(interior(ga), interior(ya), *bn, tb=tb[0].cpu(), tg=tb[1].cpu()), half_ulp_bf16=T == BF16)
    assert outside_untouched(dyp)


# --------------------------------------------------------------------------------------------------- the chain
# (B, H, W, C): the smallest shape that reaches the path named; then per (shape, with SE): relu, training, accumulate, rpp
SHAPES = [
    ((2, 6, 10, 64), "wstep > W: most threads idle", {0: (1, 1, 0, 4), 1: (1, 1, 1, 1)}),
    ((1, 5, 67, 128), "W odd: two unrolled trips + a 3-wide tail (fp32)", {0: (0, 1, 0, 2), 1: (1, 0, 0, 5)}),
    ((3, 7, 9, 1024), "cpp == 256, wstep == 1 (fp32); _apply_part's C limit", {0: (1, 1, 0, 2), 1: (1, 1, 0, 1)}),
    ((3, 7, 9, 1024), "the same, single part (rows_per_part = H + 3) / one part per image", {0: (1, 1, 0, 10), 1: (1, 1, 0, 7)}),
    ((2, 4, 6, 1280), "no-`inv` path in both dtypes; with SE: Cr = 80 > 64", {0: (1, 0, 1, 4), 1: (1, 1, 0, 1)}),
    ((2, 3, 5, 2048), "no-`inv` in fp32, `inv` in bf16", {0: (1, 1, 1, 1), 1: (0, 1, 0, 3)}),
    ((2, 4, 4, 48), "no-`inv`; cols = 96 does not divide 1024 in block_colsum", {0: (1, 1, 0, 1), 1: (1, 1, 0, 1)}),
    ((17, 4, 4, 64), "B > 16 in the stage-2 image loops", {0: (1, 0, 0, 2), 1: (1, 1, 1, 4)}),
    ((1, 2, 2, 16), "smallest SE (Cr = 1); B = 1", {0: (0, 1, 1, 1), 1: (1, 0, 1, 2)}),
]
CHAIN_CASES = [(i, T, se) for i in range(len(SHAPES)) for T in (F32, BF16) for se in (0, 1)]


def chain_case(i, T, se):
    shape, _, settings = SHAPES[i]
    return make_case(*shape, T, seed=1000 + 10 * i + se), settings[se]


@pytest.mark.parametrize("i,T,se", CHAIN_CASES, ids=[f"{'x'.join(map(str, SHAPES[i][0]))}-{'bf16' if T == BF16 else 'fp32'}-se{se}"
                                                    for i, T, se in CHAIN_CASES])
def test_chain_against_float64(dev, i, T, se):
    """reduce -> (squeeze -> excite) -> every coefficient entry point -> apply and apply_part, each against float64."""
    c, (relu, training, accumulate, rpp) = chain_case(i, T, se)
    ya, ga = upload(dev, c["y"]), upload(dev, c["dout"])
    assert torch.equal(interior(ya), c["y"])
    a = interior(ya).double() * c["scale"].double() + c["shift"].double()
    assert float(a.abs().min()) >= c["margin"]                               # the ReLU margin, on the stored values
    red = run_reduce(dev, c, ya, ga, relu, rpp)
    fwd = run_se_forward(dev, c, ya, relu, rpp) if se else None
    coefs, parts = run_coef(dev, red, c["H"], c["W"], c, training, accumulate, fwd, (c["w1"], c["w2"]) if se else None, seed=i)
    run_apply(dev, c, ya, ga, relu, coefs, parts if training else None, fwd)


@pytest.mark.parametrize("T", [F32, BF16])
def test_channel_slices_leave_their_neighbours_alone(dev, T):
    """y, dout and dy as the slice [64, 128) of 192-channel buffers: same numbers, every byte outside unchanged."""
    c = make_case(2, 5, 6, 64, T, seed=77)
    ya, ga = upload(dev, c["y"], 192, 64), upload(dev, c["dout"], 192, 64)
    red = run_reduce(dev, c, ya, ga, 1, 2)
    fwd = run_se_forward(dev, c, ya, 1, 2)
    coefs, parts = run_coef(dev, red, 5, 6, c, 1, 0, fwd, (c["w1"], c["w2"]), variants=("stage",))
    run_apply(dev, c, ya, ga, 1, coefs, parts, fwd, dy_slice=(192, 64))


ROWS_PER_IMAGE = [1, 3, 4, 5, 8, 9, 12, 15, 16, 17, 28, 33, 64]


@pytest.mark.parametrize("P", ROWS_PER_IMAGE)
def test_coefficients_from_a_slab_of_P_rows_per_image(dev, P):
    """strided_sum16's cascaded tails (16 / 8 / 4 / 1 rows at a stride of 1024 / cols lanes) and block_colsum's three
    regimes: cols = 96 (does not divide 1024), 128 (8 row lanes) and 1024 (cols >= the block). Synthetic slabs."""
    for n, (Cn, use_se) in enumerate(((48, 1), (64, 0), (64, 1), (512, P % 2))):
        B, Cr = 2, max(1, Cn // 16)
        red, bn = synthetic_slab(B, P, Cn, seed=31 * P + n)
        se = synthetic_se(B, Cn, Cr, P * 4, seed=P + n) if use_se else None
        g = torch.Generator().manual_seed(P)
        w = (torch.randn(Cr, Cn, generator=g) / math.sqrt(Cn), torch.randn(Cn, Cr, generator=g)) if use_se else None
        run_coef(dev, red.to(dev), P, 4, bn, training=1 - (P + n) % 2 * (n == 1), accumulate=(P + n) % 2, se=se, w=w, seed=P)


@pytest.mark.parametrize("rows_total", [1, 15, 16, 17, 112, 113, 128, 129, 1024])
def test_channel_parallel_coefficients_over_rows_total(dev, rows_total):
    """insar_bn_bwd_coef's 8 x 16-row unrolled fold and its tail (boundaries at 112 / 113 / 128 / 129), C = 72: a partial
    last 64-channel work-group."""
    red, bn = synthetic_slab(1, rows_total, 72, seed=rows_total)
    run_coef(dev, red.to(dev), 8, rows_total, bn, training=rows_total % 2, accumulate=rows_total // 16 % 2, variants=("bn", "coef"),
             seed=rows_total)


# --------------------------------------------------------------------------------------------------- pool form
@pytest.mark.parametrize("T", [F32, BF16])
@pytest.mark.parametrize("shape", [(2, 6, 10, 64), (1, 4, 68, 128), (2, 2, 2, 1024)])
def test_pool_form(dev, shape, T):
    """dout = round_T(dskip + (arg == position ? dpooled : 0)) inside the reduce and apply passes, arg from
    insar_bn_relu_apply_pool_arg (windows with exact ties: ReLU zeros, and equal positive values planted below)."""
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    B, H, W, Cn = shape
    c = make_case(*shape, T, seed=500 + Cn)
    y = c["y"].clone()
    y[:, 0::2, 1::2, ::3] = y[:, 0::2, 0::2, ::3]                           # (0,0) == (0,1) in every third channel ...
    y[:, 1::2, 1::2, 1::6] = y[:, 0::2, 1::2, 1::6]                         # ... and (0,1) == (1,1) in every sixth
    c["y"], c["margin"] = enforce_margin(y, c["scale"], c["shift"], T)
    ya, ga = upload(dev, c["y"]), upload(dev, c["dout"])
    fwd = run_se_forward(dev, c, ya, 1, 2)
    sc, sh, mu, istd, gate = devs(dev, c, "scale", "shift", "mean", "invstd") + [fwd["gate"].to(dev)]
    za = upload(dev, torch.zeros(B, H, W, Cn, dtype=T))
    pa = upload(dev, torch.zeros(B, H // 2, W // 2, Cn, dtype=T))
    arg = torch.full((B, H // 2, W // 2, Cn), 9, dtype=torch.uint8, device=dev)
    call("insar_bn_relu_apply_pool_arg", ya.ref, ptr(sc), ptr(sh), ptr(gate), za.ref, pa.ref, ptr(arg), 1, stream_ptr())
    torch.cuda.synchronize()
    z = interior(za)
    ref_arg = R.pool_arg(z)
    assert torch.equal(arg.cpu(), ref_arg)
    win = torch.stack([z[:, 0::2, 0::2], z[:, 0::2, 1::2], z[:, 1::2, 0::2], z[:, 1::2, 1::2]], 0)
    assert torch.equal(interior(pa), win.max(0).values)
    ties = (win == win.max(0).values).sum(0) > 1
    assert bool((ties & (win.max(0).values > 0)).any()) and bool((ties & (win.max(0).values == 0)).any())
    g = torch.Generator().manual_seed(9)
    dpool = torch.randn(B, H // 2, W // 2, Cn, generator=g).to(T)
    da = upload(dev, dpool)
    dout = R.pool_dout(c["dout"], dpool, ref_arg, T)
    rpp, P = 4, -(-H // 4)
    part = nan_buf(dev, B, P, 2, Cn)
    call("insar_bnrelu_bwd_reduce_pool", ga.ref, da.ref, ptr(arg), ya.ref, ptr(sc), ptr(sh), ptr(part), 1, rpp, stream_ptr())
    torch.cuda.synchronize()
    check("reduce_pool", part, *R.reduce(dout, c["y"], c["scale"], c["shift"], 1, rpp))
    coefs, _ = run_coef(dev, part, H, W, c, 1, 0, fwd, (c["w1"], c["w2"]), variants=("coef",))
    dya = upload(dev, torch.zeros(B, H, W, Cn, dtype=T))
    cB, k1, k2 = (coefs[k].to(dev) for k in ("coefB", "k1", "k2"))
    call("insar_bnrelu_bwd_apply_pool", ga.ref, da.ref, ptr(arg), ya.ref, ptr(sc), ptr(sh), ptr(mu), ptr(istd), ptr(gate),
         ptr(cB), ptr(k1), ptr(k2), dya.ref, 1, stream_ptr())
    torch.cuda.synchronize()
    check("dy_pool", interior(dya), *R.apply(dout, c["y"], c["scale"], c["shift"], c["mean"], c["invstd"], 1, fwd["gate"],
                                            coefs["coefB"], k1=coefs["k1"], k2=coefs["k2"]), half_ulp_bf16=T == BF16)
    assert outside_untouched(dya) and outside_untouched(ga) and outside_untouched(da)


# --------------------------------------------------------------------------------------------------- outc form
@pytest.mark.parametrize("T", [F32, BF16])
@pytest.mark.parametrize("with_wpart", [0, 1])
@pytest.mark.parametrize("with_gate", [0, 1])
@pytest.mark.parametrize("Kc", [1, 2, 3, 4])
def test_outc_form(dev, Kc, with_gate, with_wpart, T):
    """dout = round_T(sum_k dlogits * W[k][c]) recomputed inside the reduce and apply passes, and the output conv's own
    parameter-gradient partials (wpart) from the same pass, folded in float64. dlogits, W, y, scale, shift and the gate lie on
    a coarse binary grid, so both roundings to T (of dout and of z) are those of exact values: a bf16 result cannot differ
    from the reference by a rounding taken the other way."""
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    B, H, W, Cn, rpp = 2, 6, 10, 64, 4
    c = make_case(B, H, W, Cn, T, seed=900 + Kc, lattice=True)
    g = torch.Generator().manual_seed(Kc)
    dl = (torch.randint(-16, 17, (B, Kc, H, W), generator=g) / 8.0).float()
    wout = (torch.randint(-16, 17, (Kc, Cn), generator=g) / 16.0).float()
    gate_c = torch.exp2(-torch.randint(0, 4, (B, Cn), generator=g).float()) if with_gate else None
    ya = upload(dev, c["y"])
    sc, sh, mu, istd = devs(dev, c, "scale", "shift", "mean", "invstd")
    dld, wd, gd = dl.to(dev), wout.to(dev), gate_c.to(dev) if with_gate else None
    P = -(-H // rpp)
    part = nan_buf(dev, B, P, 2, Cn)
    wpart = nan_buf(dev, B * P, Kc * Cn + Kc) if with_wpart else None
    call("insar_bnrelu_bwd_reduce_outc", ptr(dld), ptr(wd), Kc, ya.ref, ptr(sc), ptr(sh), ptr(part), 1, rpp, ptr(gd), ptr(wpart),
         stream_ptr())
    torch.cuda.synchronize()
    dout, _ = R.outc_dout(dl, wout, T)
    assert torch.equal(dout, R.outc_dout(dl, wout, F64)[0]) or T == BF16       # the grid: fp32 holds the sums exactly
    check("reduce_outc", part, *R.reduce(dout, c["y"], c["scale"], c["shift"], 1, rpp))
    if with_wpart:
        ref_w, u_w = R.outc_wpart(dl, wout.shape, c["y"], c["scale"], c["shift"], gate_c, 1, rpp, T)
        check("wpart", wpart, ref_w, u_w)
        fold, ref_fold = wpart.double().sum(0).cpu(), ref_w.sum(0)             # the weight and bias gradient themselves
        check("wpart_fold", fold, ref_fold, u_w.sum(0))
    coefs, _ = run_coef(dev, part, H, W, c, 1, 0, variants=("bn",))
    dya = upload(dev, torch.zeros(B, H, W, Cn, dtype=T))
    k1, k2 = coefs["k1"].to(dev), coefs["k2"].to(dev)
    call("insar_bnrelu_bwd_apply_outc", ptr(dld), ptr(wd), Kc, ya.ref, ptr(sc), ptr(sh), ptr(mu), ptr(istd), ptr(gd), 0,
         ptr(k1), ptr(k2), dya.ref, 1, stream_ptr())
    torch.cuda.synchronize()
    check("dy_outc", interior(dya), *R.apply(dout, c["y"], c["scale"], c["shift"], c["mean"], c["invstd"], 1, gate_c, None,
                                            k1=coefs["k1"], k2=coefs["k2"]), half_ulp_bf16=T == BF16)
    assert outside_untouched(dya) and outside_untouched(ya)


# --------------------------------------------------------------------------------------------------- insar_bn_finalize
def finalize_case(Cn, rows, seed, count=None, integers=False):
    g = torch.Generator().manual_seed(seed)
    per = 8 if integers else 24                                 # pixels behind one partial row
    if integers:      # |mean| / sigma = 1000 with partials that are small integers: the float64 reference is exact
        v = 1000 + 2 * torch.randint(0, 2, (rows, per, Cn), generator=g).double() - 1
    else:
        sigma = 0.5 + torch.rand(Cn, generator=g, dtype=F64)
        v = torch.randn(rows, per, Cn, generator=g, dtype=F64) * sigma + torch.tensor([0.0, 3.0, 30.0], dtype=F64)[torch.arange(Cn) % 3] * sigma
    part = torch.stack([v.sum(1), (v * v).sum(1)], 1).float()
    p = dict(part=part, count=count or rows * per, gamma=torch.randn(Cn, generator=g) + 1.5, beta=torch.randn(Cn, generator=g),
             conv_bias=torch.randn(Cn, generator=g), running_mean=torch.randn(Cn, generator=g),
             running_var=torch.rand(Cn, generator=g) + 0.5)
    return p


def run_finalize(dev, p, training=1, with_bias=True, with_running=True, calls=1):
    from insar_unet_ca_amd._lib import InsarBnFinalize, call, ptr, stream_ptr
    Cn = p["gamma"].numel()
    mom, eps = R.f32(0.1), R.f32(1e-5)
    t = {k: p[k].to(dev) for k in ("part", "gamma", "beta", "conv_bias", "running_mean", "running_var")}
    nbt = torch.tensor([41], dtype=torch.int64, device=dev)
    out = {k: nan_buf(dev, Cn) for k in ("scale", "shift", "mean", "invstd")}
    d = InsarBnFinalize()
    d.part, d.rows, d.count, d.C, d.training = ptr(t["part"]), p["part"].shape[0], p["count"], Cn, training
    d.conv_bias = ptr(t["conv_bias"]) if with_bias else 0
    d.gamma, d.beta = ptr(t["gamma"]), ptr(t["beta"])
    if with_running:
        d.running_mean, d.running_var, d.num_batches_tracked = ptr(t["running_mean"]), ptr(t["running_var"]), ptr(nbt)
    d.momentum, d.eps = 0.1, 1e-5
    d.scale, d.shift, d.mean, d.invstd = (ptr(out[k]) for k in ("scale", "shift", "mean", "invstd"))
    rm, rv, n = (p["running_mean"], p["running_var"], 41) if with_running else (None, None, None)
    for _ in range(calls):
        call("insar_bn_finalize", C.byref(d), stream_ptr())
        torch.cuda.synchronize()
        ref, u = R.finalize(p["part"], p["count"], p["gamma"], p["beta"], p["conv_bias"] if with_bias else None, rm, rv, n, mom, eps,
                            training)
        for k in ("scale", "shift", "mean", "invstd"):
            check(f"fin_{k}", out[k], ref[k], u[k])
        if with_running:
            check("fin_running_mean", t["running_mean"], ref["running_mean"], u["running_mean"])
            check("fin_running_var", t["running_var"], ref["running_var"], u["running_var"])
            assert int(nbt) == ref["num_batches_tracked"] == n + training     # exactly once per training call
            rm, rv, n = t["running_mean"].cpu(), t["running_var"].cpu(), int(nbt)   # the next call starts from the stored values
    return {k: v.cpu() for k, v in out.items()}, ref


FINALIZE_CASES = [(1, 1), (63, 15), (64, 16), (65, 17), (1280, 127), (64, 128), (65, 129), (1, 4096), (63, 4096), (1280, 16),
                  (64, 1), (65, 127), (1, 129)]


@pytest.mark.parametrize("Cn,rows", FINALIZE_CASES)
def test_finalize_against_float64(dev, Cn, rows):
    """The 8 x 16-row unrolled fold and its tail (rows at 127 / 128 / 129), a partial last 64-channel work-group (C at
    63 / 64 / 65); conv_bias and the running statistics null and non-null; two training calls in a row."""
    p = finalize_case(Cn, rows, seed=Cn + rows)
    run_finalize(dev, p, 1, with_bias=bool(rows % 2), with_running=True, calls=2)
    run_finalize(dev, p, 1, with_bias=not rows % 2, with_running=False)
    run_finalize(dev, p, 0, with_bias=bool(Cn % 2), with_running=True, calls=2)          # eval: slabs ignored, nothing tracked


def test_finalize_of_a_single_pixel(dev):
    """count = 1: the biased variance (0) is also the unbiased one — n / (n - 1) must not be formed."""
    v = torch.tensor([[1.5, -2.25, 0.0, 3.0]])
    p = finalize_case(4, 1, seed=5)
    p.update(part=torch.stack([v, v * v], 1), count=1)
    out, ref = run_finalize(dev, p)
    assert torch.equal(out["invstd"], torch.full((4,), 1 / math.sqrt(R.f32(1e-5))).float())


def test_finalize_constant_and_negative_variance_channels(dev):
    """A constant channel: var = 0 exactly, invstd = 1 / sqrt(eps). A channel whose sum of squares was rounded below
    count * mean^2: the variance clamps to 0 instead of going negative (NaN from the square root)."""
    p = finalize_case(8, 16, seed=6)
    p["part"][:, 0, 0], p["part"][:, 1, 0] = 24 * 3.0, 24 * 9.0
    p["part"][:, 0, 1], p["part"][:, 1, 1] = 24 * 3.0, 24 * 9.0 * (1 - 1e-3)
    out, ref = run_finalize(dev, p)
    want = torch.tensor(1 / math.sqrt(R.f32(1e-5)), dtype=F64).float()
    assert out["invstd"][0] == want and out["invstd"][1] == want and out["mean"][0] == 3.0


def test_finalize_ill_conditioned(dev):
    """|mean| / sigma = 1000, partials that are small integers (exact in fp32, sums exact in float64): var = s2/n - m^2 loses
    six digits to cancellation, which the kernel's double-precision fold must absorb. On top of the rule: mean and invstd are
    one fp32 rounding of exact values, so within 2^-23 relative."""
    p = finalize_case(65, 128, seed=7, integers=True)
    assert bool((p["part"].double() == p["part"].double().round()).all()) and float(p["part"].max()) < 2 ** 24
    out, ref = run_finalize(dev, p)
    for k in ("mean", "invstd"):
        assert float(((out[k].double() - ref[k]) / ref[k]).abs().max()) <= 2.0 ** -23
    assert 990 < float((ref["mean"] * ref["invstd"]).min()) < 1010
