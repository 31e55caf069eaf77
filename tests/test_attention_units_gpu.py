"""GPU: every C-ABI entry point of SpatialAttention (csrc/spatial_attn.hip) and of the ChannelAttentionModule (csrc/cam.hip)
against the float64 reference tests/attention_ref.py, one launch at a time.

Planted cases: every tensor a launch reads (comp, z1, z2, s, g2, g1, dcomp, arg, bn[8], coef[4], the part slab of the
coefficient kernels; CAM's pool slabs, saved activations and gate) is planted by the test, so an error cannot hide behind
the launch before it. Chained cases (one per family and dtype): each launch is judged on what the previous one wrote,
read back from the device. Shapes are the smallest that reach each code path (SA_CASES, CAM_POOL_CASES, CAM_MLP_CASES).
Every ReLU pre-activation is at least 1e-3 of its tensor's maximum away from 0 (moved there before upload in the planted
cases, asserted on the read-back values in the chained ones), so kernel and reference take the same decision everywhere
and no element is left out of any comparison. Outputs are pre-filled with NaN, buffers with a sentinel; every buffer a
launch must not write is compared bit for bit with what it held before; every launch runs twice and must repeat itself
bit for bit.

Tolerance (one rule, attention_ref's docstring): |got - ref| <= K * 2^-24 * U; an output stored as bf16 may be half a bf16
ulp of the reference further off. Maxima, arg-maxima, untouched elements and cam_scatter_max are exact. K was fixed BEFORE
any kernel ran: the reference's formulas evaluated in float32 on the CPU in naive order (dt=torch.float32) on these same
planted cases, measured against float64 (floor_ratios below):
    largest float32 floor ratio per output
        sa_compress: mean 0.45   sa_conv(1): z 0.63  stat 0.18   sa_conv(2): z 0.64  stat 0.19   sa_gate: s 1.36  out 1.09
        sa_dscale: g2 0.54  part 0.12   sa_bwd_stencil(2): g1 0.61  part 0.46   sa_bwd_stencil(1): dcomp 0.69  part 0.56
        sa_bwd_coef (one rounding of a float64 fold): dgamma 0.55  dbeta 0.41  coef 0.62  dw2 0.85  db2 0.73  dw1 0.85  db1 0.55
        sa_dx 1.03   cam_pool: psum 0.88   cam_excite: avg 0.81  ha 0.08  hm 0.25  gate 1.38
        cam_bwd_coef: du 0.89  dta 0.19  dtm 0.19  coefB 0.20  dmax 0.21  dW1 0.22  dW2 0.80
    K = 2 * 1.38 = 2.76
Kernel, measured on an MI355X (largest ratio per output over all cases of this file):
        sa_compress: mean 0.45   sa_conv(1): z 0.56  stat 0.18   sa_conv(2): z 0.46  stat 0.14   sa_gate: s 1.29  out 1.09
        sa_dscale: g2 0.51  part 0.12   sa_bwd_stencil(2): g1 0.49  part 0.35   sa_bwd_stencil(1): dcomp 0.60  part 0.56
        sa_bwd_coef: dgamma 0.55  dbeta 0.43  coef 0.62  dw2 0.85  db2 0.73  dw1 0.85  db1 0.55   sa_dx 1.02
        cam_pool: psum 0.88   cam_excite: avg 0.81  ha 0.06  hm 0.04  gate 1.38
        cam_bwd_coef: du 0.89  dta 0.19  dtm 0.19  coefB 0.20  dmax 0.21  dW1 0.27  dW2 0.97
        insar_bn_finalize inside the SA chain (C = 1): mean 0.17  invstd 0.14  scale 0.07  shift 0.08
    nothing needed more than 1.38 of the 2.76 allowed; every exact output (maxima, arg-maxima, untouched elements, the
    scatter) was exact, and every launch repeated itself bit for bit. No kernel had to be changed.
"""
import ctypes as C
import functools
import math
import zlib

import pytest
import torch

from tests import attention_ref as A
from tests import bn_chain_ref as R

pytestmark = pytest.mark.gpu

K = 2.76
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


# --------------------------------------------------------------------------------------------------- shared helpers
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def enforce_margin(z, sc, sh):
    """Move every element of the fp32 map z whose pre-activation |z*sc + sh| is below 1e-3 of the map's maximum out to that
    margin (keeping its sign); returns the stored map and the margin, asserted on the stored values."""
    z, sc, sh = z.float(), float(sc), float(sh)
    a = z.double() * sc + sh
    margin = 1e-3 * float(a.abs().max())
    sgn = torch.where(a >= 0, 1.0, -1.0).double()
    for i in range(1, 40):
        bad = (z.double() * sc + sh).abs() < margin
        if not bool(bad.any()):
            break
        z = torch.where(bad, ((sgn * (1.0 + i * i) * margin - sh) / sc).float(), z)
    assert_margin(z, sc, sh, margin)
    return z, margin


def assert_margin(z, sc, sh, margin=None):
    a = (z.double() * float(sc) + float(sh)).abs()
    margin = 1e-3 * float(a.max()) if margin is None else margin
    assert float(a.min()) >= margin > 0, (float(a.min()), margin)


def upload(dev, t, Ctot=None, c_off=0):
    """NHWC tensor -> Act slice [c_off, c_off + C) of a padded buffer whose every other element holds a sentinel."""
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
    """Every element outside the slice's interior (halo, neighbouring slices) still holds the sentinel."""
    b = a.buf.clone()
    b[:, 1:-1, 1:-1, a.c_off:a.c_off + a.c_len] = SENTINEL
    return bool((b == SENTINEL).all())


def bits(t):
    """The tensor's bit pattern on the CPU (NaN-safe equality)."""
    t = t.detach().contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same(a, b):
    return torch.equal(bits(a), bits(b))


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


def exact(name, got, ref):
    """Equal values everywhere, NaN where and only where the reference has one."""
    got = got.detach().cpu().reshape(ref.shape).to(ref.dtype)
    nan = torch.isnan(ref) if ref.is_floating_point() else torch.zeros(ref.shape, dtype=torch.bool)
    assert torch.equal(torch.isnan(got) if got.is_floating_point() else nan, nan) and bool((got == ref)[~nan].all()), name


def twice(prep, launch, outs):
    """Run prep + launch twice; the outputs (callables returning tensors) must agree bit for bit."""
    seen = []
    for _ in range(2):
        prep()
        launch()
        torch.cuda.synchronize()
        seen.append([bits(o()).clone() for o in outs])
    for a, b in zip(*seen):
        assert torch.equal(a, b)


def untouched(before, after, skip=()):
    for k in before:
        if k not in skip:
            assert same(before[k], after[k]), k


# =================================================================================================== SpatialAttention
# name: (B, H, W, C, dtype, rows, training, (Ctot, c_off) or None, launches or None = all, pattern)
SA_ALL = ("compress", "conv1", "conv2", "gate", "dscale", "coef2", "stencil2", "coef1", "stencil1", "coef0", "dx")
SA_CASES = {
    # lanes per pixel: bf16 C = 8, 16, 24, 40, 136, 1024 (L = 1, 2, 2, 4, 16, 16; chunks 1, 2, 3, 5, 17, 128)
    "bf16-C1024-W20-H5-rows3of10-items2560": (2, 5, 20, 1024, BF16, 3, 1, None, None, "noise"),
    "bf16-C64-W300-H2-rowsBH-items2400": (1, 2, 300, 64, BF16, 2, 1, None, None, "noise"),
    "bf16-C8-W3-H1-rows5gtBH-eval": (2, 1, 3, 8, BF16, 5, 0, None, None, "noise"),
    "bf16-C16-W1-H5-rows1": (1, 5, 1, 16, BF16, 1, 1, None, None, "noise"),
    "bf16-C24-W3-H2-rows3of4": (2, 2, 3, 24, BF16, 3, 1, None, None, "noise"),
    "bf16-C40-W20-H5-rowsBH-slice0of80": (2, 5, 20, 40, BF16, 10, 1, (80, 0), None, "noise"),
    "bf16-C136-W3-H2-rows1-slice136of272-eval": (1, 2, 3, 136, BF16, 1, 0, (272, 136), None, "noise"),
    # fp32 C = 8, 24, 64 (L = 2, 4, 16; chunks 2, 6, 16)
    "fp32-C8-W20-H5-rows3of10": (2, 5, 20, 8, F32, 3, 1, None, None, "noise"),
    "fp32-C24-W300-H2-rows7gtBH": (2, 2, 300, 24, F32, 7, 1, None, None, "noise"),
    "fp32-C64-W1-H1-rows2of3": (3, 1, 1, 64, F32, 2, 1, None, None, "noise"),
    "fp32-C64-W3-H5-rows4of10-slice64of128": (2, 5, 3, 64, F32, 4, 1, (128, 64), None, "noise"),
    "fp32-C24-W20-H2-rowsBH-slice0of48-eval": (2, 2, 20, 24, F32, 4, 0, (48, 0), None, "noise"),
    # the 16384 work-group cap of compress, gate and dx: a grid-stride second trip
    "bf16-C8-W1-H16400-gridcap": (1, 16400, 1, 8, BF16, 4096, 1, None, ("compress", "gate", "dx"), "noise"),
    # stencil taps: a delta at the last pixel of image 0 and the first of image 1; a map that lives on the image border only
    "fp32-C8-W20-H5-rows3of10-delta": (2, 5, 20, 8, F32, 3, 1, None, ("conv1", "conv2", "stencil2", "stencil1"), "delta"),
    "fp32-C8-W20-H5-rows3of10-border": (2, 5, 20, 8, F32, 3, 1, None, ("conv1", "conv2", "stencil2", "stencil1"), "border"),
    "fp32-C8-W300-H2-rows1-border": (2, 2, 300, 8, F32, 1, 0, None, ("conv1", "conv2", "stencil2", "stencil1"), "border"),
}
SA_PARAMS = [(n, l) for n, v in SA_CASES.items() for l in (v[8] or SA_ALL)]
# chained cases: the inputs (x, dy, weights) come from here, everything else from the device. The suffix seeds the inputs: it
# was chosen so that every BatchNorm output the kernels produce clears the ReLU margin (asserted on the read-back values).
SA_CHAIN_CASES = {
    "bf16-C40-W7-H5-rows3of10-slice40of80-s7": (2, 5, 7, 40, BF16, 3, 1, (80, 40), None, "noise"),
    "fp32-C24-W7-H5-rows4of10-s5": (2, 5, 7, 24, F32, 4, 1, None, None, "noise"),
}


@functools.lru_cache(maxsize=None)
def sa_case(name):
    """The planted tensors of one SA case (CPU, stored dtypes)."""
    B, H, W, Cn, T, rows, training, sl, _, pattern = (SA_CASES.get(name) or SA_CHAIN_CASES[name])
    g = _gen(name)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    M, CH = B * H * W, 8 if T == BF16 else 4
    c = dict(name=name, B=B, H=H, W=W, C=Cn, T=T, rows=rows, training=training, slice=sl, M=M)
    x = (rn(B, H, W, Cn) * (0.5 + torch.rand(Cn, generator=g, dtype=F64))).to(T)
    xf = x.view(M, Cn)
    m, a = xf.float().max(1)
    tie = torch.arange(M) % 3 == 0                          # every third pixel holds its maximum twice: the first channel wins
    xf[tie, ((a + Cn // 2 + 3) % Cn)[tie]] = m[tie].to(T)
    assert int((xf.float() == xf.float().amax(1, keepdim=True)).sum(1).max()) >= 2
    c["x"], c["dy"] = x, rn(B, H, W, Cn).to(T)
    c["w1"], c["w2"] = (0.4 * rn(1, 2, 3, 3)).float(), (0.6 * rn(1, 1, 3, 3)).float()
    z1, z2 = (1.3 * rn(B, H, W) + 0.2).float(), (0.8 * rn(B, H, W) - 0.4).float()
    bn = []
    for z, gamma, beta in ((z1, 1.2, 0.3), (z2, -0.9, 0.2)):
        mean, inv = float(z.double().mean()), 1 / math.sqrt(float(z.double().var(unbiased=False)) + 1e-5) if M > 1 else 1.0
        bn += [gamma * inv, beta - mean * gamma * inv, mean, inv]
    c["comp"] = rn(B, H, W, 2).float()
    c["g2"], c["g1"], c["dcomp"] = rn(B, H, W).float(), rn(B, H, W).float(), rn(B, H, W, 2).float()
    c["coef"] = (0.05 * rn(4)).float() if training else torch.zeros(4)
    if pattern != "noise":
        P = torch.zeros(B, H, W, dtype=F64)
        if pattern == "delta":
            P[0, H - 1, W - 1], P[1, 0, 0] = 1.5, -2.0
        else:
            edge = torch.zeros(H, W, dtype=torch.bool)
            edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
            P = torch.where(edge, rn(B, H, W) + 3.0, P)
        P = P.float()
        c["comp"] = torch.stack([P, -0.5 * P], -1)
        z1 = torch.where(P != 0, P.abs(), torch.full_like(P, -1.0))          # ReLU(z1) = |P|
        bn[:4] = [1.0, 0.0, 0.0, 1.0]
        c["g2"], c["g1"], c["coef"] = P, P, torch.zeros(4)
    c["bn"] = torch.tensor(bn, dtype=F64).float()
    c["z1"], c["margin1"] = enforce_margin(z1, c["bn"][0], c["bn"][1])
    c["z2"], c["margin2"] = enforce_margin(z2, c["bn"][4], c["bn"][5])
    c["z1on"] = c["z1"].abs() + 1.0 if pattern != "noise" else c["z1"]      # stencil(2) of a pattern: every BN1 mask open
    c["s"] = torch.sigmoid(rn(B, H, W).clamp_min(0)).float()
    special = torch.tensor([0, CH - 1, Cn - CH, Cn - 1])                     # first / last chunk, first / last element of a chunk
    p = torch.arange(M)
    c["arg"] = torch.where(p % 2 == 0, special[(p // 2) % 4], torch.randint(0, Cn, (M,), generator=g)).reshape(B, H, W)
    c["part"] = (rn(rows, A.SA_PART_COLS) * (1 + 5 * torch.rand(A.SA_PART_COLS, generator=g, dtype=F64)) + 0.3).float()
    return c


def sa_ref(c, launch, dt=F64):
    """The reference of one launch on the planted tensors it reads."""
    rows, tr = c["rows"], c["training"]
    if launch == "compress":
        return A.sa_compress(c["x"], dt)
    if launch == "conv1":
        return A.sa_conv(1, c["comp"], c["w1"], c["bn"], rows, tr, dt)
    if launch == "conv2":
        return A.sa_conv(2, c["z1"], c["w2"], c["bn"], rows, tr, dt)
    if launch == "gate":
        return A.sa_gate(c["x"], c["z2"], c["bn"], dt)
    if launch == "dscale":
        return A.sa_dscale(c["x"], c["dy"], c["z2"], c["s"], c["bn"], rows, dt)
    if launch.startswith("coef"):
        return A.sa_bwd_coef(int(launch[4]), c["part"], c["M"], tr, dt)
    if launch == "stencil2":
        return A.sa_bwd_stencil(2, c["g2"], c["z2"], c["bn"], c["coef"][:2], c["w2"], c["z1on"], rows, dt)
    if launch == "stencil1":
        return A.sa_bwd_stencil(1, c["g1"], c["z1"], c["bn"], c["coef"][2:], c["w1"], c["comp"], rows, dt)
    return A.sa_dx(c["dy"], c["s"], c["dcomp"], c["arg"], dt)


class SaDev:
    """Device buffers of one SA unit with the planted tensors uploaded, and its descriptor."""
    MAPS = ("z1", "z2", "s", "g2", "g1", "dcomp", "part", "bn", "coef", "w1", "w2")
    GRADS = dict(dw1=18, db1=1, dgamma1=1, dbeta1=1, dw2=9, db2=1, dgamma2=1, dbeta2=1)

    def __init__(self, dev, c, z1=None):
        B, H, W, rows = c["B"], c["H"], c["W"], c["rows"]
        self.c, self.dev = c, dev
        sl = c["slice"] or ()
        self.xa, self.ya = upload(dev, c["x"], *sl), upload(dev, c["dy"], *sl)
        self.t = {k: c[k].to(dev).contiguous() for k in self.MAPS}
        if z1 is not None:
            self.t["z1"] = z1.to(dev).contiguous()
        self.t["comp"] = torch.zeros(B, H + 2, W + 2, 2, dtype=F32, device=dev)
        self.t["comp"][:, 1:-1, 1:-1] = c["comp"].to(dev)
        self.t["arg"] = c["arg"].to(torch.int16).to(dev).contiguous()
        self.t["stat1"], self.t["stat2"] = nan_buf(dev, rows, 2), nan_buf(dev, rows, 2)
        for k, n in self.GRADS.items():
            self.t[k] = nan_buf(dev, n)

    def desc(self, with_db=True):
        from insar_unet_ca_amd._lib import InsarSa, ptr
        d = InsarSa()
        d.x, d.y = self.xa.desc, self.ya.desc
        for k in ("comp", "arg", "z1", "z2", "s", "g2", "g1", "dcomp", "stat1", "stat2", "part", "w1", "w2", "bn", "coef", *self.GRADS):
            setattr(d, k, ptr(self.t[k]))
        if not with_db:
            d.db1, d.db2 = 0, 0
        d.rows, d.training = self.c["rows"], self.c["training"]
        return d

    def snapshot(self):
        s = {k: v.clone() for k, v in self.t.items()}
        s["xbuf"], s["ybuf"] = self.xa.buf.clone(), self.ya.buf.clone()
        return s


SA_ENTRY = dict(compress=("insar_sa_compress",), conv1=("insar_sa_conv", 1), conv2=("insar_sa_conv", 2), gate=("insar_sa_gate",),
                dscale=("insar_sa_dscale",), coef2=("insar_sa_bwd_coef", 2), coef1=("insar_sa_bwd_coef", 1), coef0=("insar_sa_bwd_coef", 0),
                stencil2=("insar_sa_bwd_stencil", 2), stencil1=("insar_sa_bwd_stencil", 1), dx=("insar_sa_dx",))
# the buffers a launch writes (all of it, or the columns / entries listed in sa_judge)
SA_WRITES = dict(compress=("comp", "arg"), conv1=("z1", "stat1"), conv2=("z2", "stat2"), gate=("s", "ybuf"), dscale=("g2", "part"),
                 coef2=("dgamma2", "dbeta2", "coef"), coef1=("dgamma1", "dbeta1", "coef", "dw2", "db2"), coef0=("dw1", "db1"),
                 stencil2=("g1", "part"), stencil1=("dcomp", "part"), dx=("ybuf",))


def sa_launch(D, launch, with_db=True, chain=False):
    """Pre-fill the launch's outputs (NaN; a planted slab keeps its planted values outside the columns written), run it
    twice, hold every other buffer to its bits; returns the buffers before the launch. chain: the slab and coef hold what
    the launches before wrote, so they are pre-filled with NaN as well."""
    from insar_unet_ca_amd._lib import call, stream_ptr
    c, t = D.c, D.t
    before = {}

    def prep():
        for k in SA_WRITES[launch]:
            if k == "comp":
                t[k][:, 1:-1, 1:-1] = float("nan")
            elif k == "arg":
                t[k].fill_(-1)
            elif k == "ybuf":
                y = c["dy"] if launch == "dx" else torch.full_like(c["dy"], float("nan"))
                D.ya.buf[:, 1:-1, 1:-1, D.ya.c_off:D.ya.c_off + D.ya.c_len] = y.to(D.dev)
            elif k in ("part", "coef") and not chain:
                t[k].copy_(c[k])
            else:
                t[k].fill_(float("nan"))
        before.update(D.snapshot())

    d = D.desc(with_db)
    entry = SA_ENTRY[launch]
    outs = [(lambda k=k: D.ya.buf if k == "ybuf" else t[k]) for k in SA_WRITES[launch]]
    twice(prep, lambda: call(entry[0], C.byref(d), *entry[1:], stream_ptr()), outs)
    untouched(before, D.snapshot(), skip=SA_WRITES[launch] if c["training"] or launch not in ("conv1", "conv2")
              else [k for k in SA_WRITES[launch] if not k.startswith("stat")])          # eval: stat1 / stat2 stay as they were
    assert outside_untouched(D.xa) and outside_untouched(D.ya)
    return before


def sa_judge(D, launch, ref, unit, before, with_db=True):
    """Compare what the launch wrote with the reference (ref, unit: attention_ref's values and units of this launch)."""
    c, t = D.c, D.t
    bf = c["T"] == BF16
    tag = lambda k: f"sa_{launch}.{k}"
    if launch == "compress":
        comp = t["comp"].cpu()
        check(tag("mean"), comp[:, 1:-1, 1:-1, 0], ref["mean"], unit["mean"])
        exact(tag("max"), comp[:, 1:-1, 1:-1, 1], ref["max"].float())
        exact(tag("arg"), t["arg"].cpu().to(torch.int64) & 0xFFFF, ref["arg"])
        halo = comp.clone()
        halo[:, 1:-1, 1:-1] = 0
        assert not bool(halo.any())
    elif launch in ("conv1", "conv2"):
        n = launch[4]
        check(tag("z"), t["z" + n], ref["z"], unit["z"])
        if c["training"]:
            check(tag("stat"), t["stat" + n], ref["stat"], unit["stat"])
    elif launch == "gate":
        check(tag("s"), t["s"], ref["s"], unit["s"])
        check(tag("out"), interior(D.ya), ref["out"], unit["out"], half_ulp_bf16=bf)
    elif launch == "dscale":
        check(tag("g2"), t["g2"], ref["g2"], unit["g2"])
        check(tag("part"), t["part"][:, :2], ref["part"], unit["part"])
        assert same(t["part"][:, 2:], before["part"][:, 2:])
    elif launch.startswith("coef"):
        stage = int(launch[4])
        for k in ref:
            if k == "coef":
                o = 0 if stage == 2 else 2
                check(tag(k), t["coef"][o:o + 2], ref[k], unit[k])
                assert same(t["coef"][2 - o:4 - o], before["coef"][2 - o:4 - o])
            elif k in ("db1", "db2") and not with_db:
                assert bool(torch.isnan(t[k]).all())
            else:
                check(tag(k), t[k], ref[k], unit[k])
    elif launch == "stencil2":
        check(tag("g1"), t["g1"], ref["g1"], unit["g1"])
        check(tag("part"), t["part"][:, :12], ref["part"], unit["part"])
        assert same(t["part"][:, 12:], before["part"][:, 12:])
    elif launch == "stencil1":
        check(tag("dcomp"), t["dcomp"], ref["dcomp"], unit["dcomp"])
        check(tag("part"), t["part"][:, :19], ref["part"], unit["part"])
        assert same(t["part"][:, 19:], before["part"][:, 19:])
    else:
        check(tag("dx"), interior(D.ya), ref, unit, half_ulp_bf16=bf)


@pytest.mark.parametrize("name,launch", SA_PARAMS, ids=[f"{l}-{n}" for n, l in SA_PARAMS])
def test_sa_launch_on_planted_inputs(dev, name, launch):
    c = sa_case(name)
    assert_margin(c["z1"], c["bn"][0], c["bn"][1], c["margin1"])
    assert_margin(c["z2"], c["bn"][4], c["bn"][5], c["margin2"])
    ref, unit = sa_ref(c, launch)
    for with_db in ((True, False) if launch in ("coef1", "coef0") else (True,)):
        D = SaDev(dev, c, z1=c["z1on"] if launch == "stencil2" else None)
        before = sa_launch(D, launch, with_db)
        sa_judge(D, launch, ref, unit, before, with_db)


def test_sa_refusals(dev):
    from insar_unet_ca_amd._lib import InsarError, call, stream_ptr
    c = sa_case("fp32-C8-W20-H5-rows3of10")
    D = SaDev(dev, c)
    for rows in (0, 4097):
        d = D.desc()
        d.rows = rows
        with pytest.raises(InsarError, match="1001"):
            call("insar_sa_conv", C.byref(d), 1, stream_ptr())
    d = D.desc()
    d.x.c_len = 4
    with pytest.raises(InsarError, match="1001"):
        call("insar_sa_compress", C.byref(d), stream_ptr())


# --------------------------------------------------------------------------------------------------- SA, chained
def _finalize(dev, stat, rows, count, gamma, beta, bias, bn, k):
    """insar_bn_finalize (C = 1, training, no running statistics) into bn[4k : 4k+4]; judged against bn_chain_ref."""
    from insar_unet_ca_amd._lib import InsarBnFinalize, call, ptr, stream_ptr
    p = [torch.tensor([v], dtype=F32, device=dev) for v in (gamma, beta, bias)]
    d = InsarBnFinalize()
    d.part, d.rows, d.count, d.C, d.training = ptr(stat), rows, count, 1, 1
    d.gamma, d.beta, d.conv_bias = ptr(p[0]), ptr(p[1]), ptr(p[2])
    d.momentum, d.eps = 0.1, 1e-5
    base = bn.data_ptr() + 16 * k
    d.scale, d.shift, d.mean, d.invstd = base, base + 4, base + 8, base + 12
    call("insar_bn_finalize", C.byref(d), stream_ptr())
    torch.cuda.synchronize()
    ref, u = R.finalize(stat.cpu().reshape(rows, 2, 1), count, p[0].cpu(), p[1].cpu(), p[2].cpu(), None, None, None, R.f32(0.1), R.f32(1e-5), 1)
    for i, key in enumerate(("scale", "shift", "mean", "invstd")):
        check(f"sa_chain.finalize.{key}", bn[4 * k + i], ref[key].reshape(()), u[key].reshape(()))


@pytest.mark.parametrize("name", list(SA_CHAIN_CASES))
def test_sa_chain_each_launch_on_what_the_previous_one_wrote(dev, name):
    """compress -> conv(1) -> finalize -> conv(2) -> finalize -> gate -> dscale -> coef(2) -> stencil(2) -> coef(1) -> stencil(1)
    -> coef(0) -> dx; the reference of each launch reads the device's own intermediate tensors."""
    c = dict(sa_case(name))
    B, H, W, rows, M = c["B"], c["H"], c["W"], c["rows"], c["M"]
    D = SaDev(dev, c)
    for k in ("z1", "z2", "s", "g2", "g1", "dcomp", "coef", "bn", "part", "stat1", "stat2"):
        D.t[k].fill_(float("nan"))
    cpu = lambda k: D.t[k].cpu()
    run = lambda launch, ref, **kw: sa_judge(D, launch, *ref, sa_launch(D, launch, **kw))

    run("compress", A.sa_compress(c["x"]), chain=True)
    comp = cpu("comp")[:, 1:-1, 1:-1]
    run("conv1", A.sa_conv(1, comp, c["w1"], None, rows, 1), chain=True)
    _finalize(dev, D.t["stat1"], rows, M, 1.2, 0.3, 0.7, D.t["bn"], 0)
    bn = cpu("bn")
    assert_margin(cpu("z1"), bn[0], bn[1])
    run("conv2", A.sa_conv(2, cpu("z1"), c["w2"], bn, rows, 1), chain=True)
    _finalize(dev, D.t["stat2"], rows, M, -0.9, 0.2, -0.4, D.t["bn"], 1)
    bn = cpu("bn")
    assert_margin(cpu("z2"), bn[4], bn[5])
    run("gate", A.sa_gate(c["x"], cpu("z2"), bn), chain=True)
    s = cpu("s")
    assert 0 < float((s > 0.5).float().mean()) < 1
    D.ya.buf[:, 1:-1, 1:-1, D.ya.c_off:D.ya.c_off + D.ya.c_len] = c["dy"].to(dev)      # backward: y holds d out
    run("dscale", A.sa_dscale(c["x"], c["dy"], cpu("z2"), s, bn, rows), chain=True)
    run("coef2", A.sa_bwd_coef(2, cpu("part"), M, 1), chain=True)
    run("stencil2", A.sa_bwd_stencil(2, cpu("g2"), cpu("z2"), bn, cpu("coef")[:2], c["w2"], cpu("z1"), rows), chain=True)
    run("coef1", A.sa_bwd_coef(1, cpu("part"), M, 1), chain=True)
    run("stencil1", A.sa_bwd_stencil(1, cpu("g1"), cpu("z1"), bn, cpu("coef")[2:], c["w1"], comp, rows), chain=True)
    run("coef0", A.sa_bwd_coef(0, cpu("part"), M, 1), chain=True)
    arg = (cpu("arg").to(torch.int64) & 0xFFFF).reshape(B, H, W)
    run("dx", A.sa_dx(c["dy"], s, cpu("dcomp"), arg), chain=True)


# =================================================================================================== ChannelAttentionModule
# name: (dtype, B, H, W, C, rows_per_part); cpp = C / (8 | 4) chunks per pixel, wstep = 256 / cpp
CAM_POOL_CASES = {
    "bf16-C8-cpp1-W5-rpp1": (BF16, 2, 7, 5, 8, 1),
    "bf16-C8-cpp1-W40-rpp3": (BF16, 2, 7, 40, 8, 3),
    "bf16-C64-cpp8-W40gtwstep-rpp2": (BF16, 2, 7, 40, 64, 2),
    "bf16-C64-cpp8-W1-rppH": (BF16, 3, 7, 1, 64, 7),
    "bf16-C256-cpp32-W40gtwstep-rpp3": (BF16, 2, 7, 40, 256, 3),
    "bf16-C256-cpp32-W5-rppgtH": (BF16, 1, 7, 5, 256, 9),
    "bf16-C2048-cpp256-W5-rpp2": (BF16, 2, 7, 5, 2048, 2),
    "bf16-C2048-cpp256-W1-rpp1": (BF16, 1, 7, 1, 2048, 1),
    "fp32-C4-cpp1-W40-rpp3": (F32, 2, 7, 40, 4, 3),
    "fp32-C4-cpp1-W300gtwstep-rpp2": (F32, 1, 7, 300, 4, 2),
    "fp32-C256-cpp64-W5gtwstep-rpp2": (F32, 2, 7, 5, 256, 2),
    "fp32-C256-cpp64-W1-rppgtH": (F32, 2, 7, 1, 256, 8),
    "fp32-C1024-cpp256-W5-rpp3": (F32, 2, 7, 5, 1024, 3),
    "fp32-C1024-cpp256-W40-rppH": (F32, 1, 7, 40, 1024, 7),
}


@functools.lru_cache(maxsize=None)
def cam_pool_case(name, with_nan=False):
    T, B, H, W, Cn, rpp = CAM_POOL_CASES[name]
    g = _gen(name)
    x = (torch.randn(B, H, W, Cn, generator=g, dtype=F64) * (0.5 + torch.rand(Cn, generator=g, dtype=F64))).to(T)
    wstep = max(1, 256 // (Cn // (8 if T == BF16 else 4)))
    top = (x.float().amax((1, 2)) + 1.0).to(T)                               # [B][C], above everything else in the channel
    ch = torch.arange(Cn)
    w0, w1 = min(1, W - 1), min(2, W - 1)

    def plant(sel, spots):
        for h, w in spots:
            x[:, h, w, :] = torch.where(sel[None, :], top, x[:, h, w, :])
    plant(ch % 8 == 1, [(3, w0), (3, w1)])                                   # neighbouring threads of one part (W > 1)
    plant(ch % 8 == 2, [(0, W - 1), (H - 1, 0)])                             # first and last part; the later one has the smaller w
    plant(ch % 8 == 3, [(0, w0), (1, w0)])                                   # one thread's share, rows of one part (rpp > 1)
    plant(ch % 8 == 5, [(2, 0), (2, min(wstep, W - 1))])                     # one thread's share along w (W > wstep)
    plant(ch % 8 == 6, [(2, W - 1), (3, 0), (5, w0)])                        # three parts (rpp <= 2)
    xf = x.float().reshape(B, H * W, Cn)
    assert int((xf == xf.amax(1, keepdim=True)).sum(1).max()) >= 2
    if with_nan:                                                             # one NaN per (image, channel)
        pos = torch.randint(0, H * W, (B, Cn), generator=g)
        x.view(B, H * W, Cn).scatter_(1, pos[:, None, :], float("nan"))
    return dict(T=T, B=B, H=H, W=W, C=Cn, rpp=rpp, x=x, P=-(-H // rpp))


def cam_desc(dev, B, H, W, Cn, Cr, rows, tensors, accumulate=0):
    from insar_unet_ca_amd._lib import InsarCam, ptr
    d = InsarCam()
    d.B, d.H, d.W, d.C, d.Cr, d.rows, d.accumulate = B, H, W, Cn, Cr, rows, accumulate
    for k, v in tensors.items():
        setattr(d, k, ptr(v))
    return d


def cam_out_buffers(dev, B, Cn, Cr):
    t = {k: nan_buf(dev, B, Cn) for k in ("avg", "mx", "gate", "coefB", "dmax")}
    t.update(ha=nan_buf(dev, B, Cr), hm=nan_buf(dev, B, Cr), ws=nan_buf(dev, B * (Cn + 2 * Cr)),
             arg=torch.full((B, Cn), -7, dtype=torch.int32, device=dev), dw1=nan_buf(dev, Cr, Cn), dw2=nan_buf(dev, Cn, Cr))
    return t


def run_cam_pool(dev, c, xa):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    B, P, Cn = c["B"], c["P"], c["C"]
    o = dict(psum=nan_buf(dev, B, P, Cn), pmax=nan_buf(dev, B, P, Cn), parg=torch.empty(B, P, Cn, dtype=torch.int32, device=dev))

    def prep():
        o["psum"].fill_(float("nan")), o["pmax"].fill_(float("nan")), o["parg"].fill_(-7)
    xbuf = xa.buf.clone()
    twice(prep, lambda: call("insar_cam_pool", xa.ref, ptr(o["psum"]), ptr(o["pmax"]), ptr(o["parg"]), c["rpp"], stream_ptr()),
          [lambda k=k: o[k] for k in o])
    assert same(xbuf, xa.buf)
    return o


@pytest.mark.parametrize("with_nan", [False, True], ids=["ties", "one-nan-per-channel"])
@pytest.mark.parametrize("name", list(CAM_POOL_CASES))
def test_cam_pool_and_fold(dev, name, with_nan):
    """insar_cam_pool on planted ties (one thread's share, threads of a part, parts), then insar_cam_excite's fold of those
    slabs: pmax, parg, mx and arg exact, the first maximum in scan order (h, then w); a NaN is the maximum."""
    from insar_unet_ca_amd._lib import call, stream_ptr
    c = cam_pool_case(name, with_nan)
    B, H, W, Cn, P, T = c["B"], c["H"], c["W"], c["C"], c["P"], c["T"]
    sl = (2 * Cn, Cn) if Cn <= 256 else ()                                  # a channel slice of a buffer twice as wide
    xa = upload(dev, c["x"], *sl)
    o = run_cam_pool(dev, c, xa)
    ref, unit = A.cam_pool(c["x"], c["rpp"])
    exact("cam_pool.pmax", o["pmax"], ref["pmax"].float())
    exact("cam_pool.parg", o["parg"].cpu().to(torch.int64), ref["parg"])
    nan = torch.isnan(ref["psum"])
    assert torch.equal(torch.isnan(o["psum"].cpu()), nan) and bool(nan.any()) == with_nan
    check("cam_pool.psum", o["psum"].cpu().nan_to_num(0.0), ref["psum"].nan_to_num(0.0), unit["psum"].nan_to_num(0.0))
    Cr = max(1, Cn // 16)
    g = _gen(name + "w")
    w1, w2 = (torch.randn(Cr, Cn, generator=g) / math.sqrt(Cn)).to(dev), torch.randn(Cn, Cr, generator=g).to(dev)
    t = cam_out_buffers(dev, B, Cn, Cr)
    d = cam_desc(dev, B, H, W, Cn, Cr, P, dict(t, psum=o["psum"], pmax=o["pmax"], parg=o["parg"], w1=w1, w2=w2))
    call("insar_cam_excite", C.byref(d), stream_ptr())
    torch.cuda.synchronize()
    ex, _ = A.cam_excite(o["psum"].cpu(), o["pmax"].cpu(), o["parg"].cpu(), w1.cpu(), w2.cpu(), H, W)
    exact("cam_excite.mx", t["mx"], ex["mx"].float())
    exact("cam_excite.arg", t["arg"].cpu().to(torch.int64), ex["arg"])
    xf = c["x"].double().reshape(B, H * W, Cn)
    m, a = A._first_max(xf, 1)
    exact("cam.mx of x", t["mx"], m.float())
    exact("cam.arg of x", t["arg"].cpu().to(torch.int64), a)
    if with_nan:
        assert bool(torch.isnan(t["mx"]).all()) and bool(torch.isnan(xf.gather(1, t["arg"].cpu().long()[:, None, :])).all())


def test_cam_pool_refusals(dev):
    from insar_unet_ca_amd._lib import InsarError, call, ptr, stream_ptr
    for T, Cn, rpp in ((BF16, 24, 1), (F32, 2048, 1), (BF16, 64, 0)):
        xa = upload(dev, torch.zeros(1, 2, 2, Cn, dtype=T))
        o = [nan_buf(dev, 1, 2, Cn), nan_buf(dev, 1, 2, Cn), torch.zeros(1, 2, Cn, dtype=torch.int32, device=dev)]
        with pytest.raises(InsarError, match="1001"):
            call("insar_cam_pool", xa.ref, ptr(o[0]), ptr(o[1]), ptr(o[2]), rpp, stream_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isnan(o[0]).all())


# name: (C, Cr, B, rows, accumulate)
CAM_MLP_CASES = {
    "C8-Cr1-B1-rows1": (8, 1, 1, 1, 0),
    "C40-Cr4-B3-rows3-acc": (40, 4, 3, 3, 1),
    "C256-Cr16-B1-rows64": (256, 16, 1, 64, 0),
    "C256-Cr16-B3-rows64-acc": (256, 16, 3, 64, 1),
    "C1600-Cr100-B3-rows3-acc": (1600, 100, 3, 3, 1),
    "C1600-Cr100-B1-rows1": (1600, 100, 1, 1, 0),
}


@functools.lru_cache(maxsize=None)
def cam_mlp_case(name):
    Cn, Cr, B, rows, acc = CAM_MLP_CASES[name]
    g = _gen(name)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    H, W = 2 * rows, 5
    c = dict(C=Cn, Cr=Cr, B=B, rows=rows, acc=acc, H=H, W=W)
    c["psum"] = (rn(B, rows, Cn) * 2 * W + 0.5 * W).float()
    pmax = (rn(B, rows, Cn) + 1.0).float()
    if rows > 1:                                       # the maximum of every other channel sits in two parts: the first one wins
        top = pmax.amax(1) + 0.5
        pmax[:, rows // 2, 0::2], pmax[:, rows - 1, 0::2] = top[:, 0::2], top[:, 0::2]
    c["pmax"] = pmax
    c["parg"] = (torch.randint(0, 2 * W, (B, rows, Cn), generator=g) + 2 * W * torch.arange(rows)[None, :, None]).to(torch.int32)
    c["w1"], c["w2"] = (rn(Cr, Cn) / math.sqrt(Cn)).float(), (rn(Cn, Cr) * 2 / math.sqrt(Cr)).float()
    for _ in range(50):                                # hidden pre-activations clear of 0: re-draw the weight rows that are not
        ex, _ = A.cam_excite(c["psum"], c["pmax"], c["parg"], c["w1"], c["w2"], H, W)
        pre = torch.cat([ex["pre_a"], ex["pre_m"]], 0)
        c["margin"] = 1e-3 * float(pre.abs().max())
        bad = (pre.abs() < c["margin"]).any(0)
        if not bool(bad.any()):
            break
        c["w1"][bad] = (rn(int(bad.sum()), Cn) / math.sqrt(Cn)).float()
    # backward: planted saved activations, any values of the right kind
    c["red"] = rn(B, rows, 2, Cn).float()
    c["gate"] = torch.sigmoid(rn(B, Cn)).float()
    c["avg"], c["mx"] = rn(B, Cn).float(), (rn(B, Cn) + 1.0).float()
    for k in ("ha", "hm"):
        v = rn(B, Cr)
        m = 1e-3 * float(v.abs().max())
        c[k] = torch.where(v.abs() < m, torch.full_like(v, m), v).clamp_min(0).float()
        assert float(c[k][c[k] > 0].min()) >= m * (1 - 1e-6) if bool((c[k] > 0).any()) else True
    c["dw1_0"], c["dw2_0"] = rn(Cr, Cn).float(), rn(Cn, Cr).float()
    return c


def cam_excite_ref(c, dt=F64):
    return A.cam_excite(c["psum"], c["pmax"], c["parg"], c["w1"], c["w2"], c["H"], c["W"], dt)


def cam_bwd_ref(c, dt=F64):
    return A.cam_bwd_coef(c["red"], c["gate"], c["ha"], c["hm"], c["avg"], c["mx"], c["w1"], c["w2"], c["H"], c["W"], dt)


def judge_excite(t, ref, unit):
    exact("cam_excite.mx", t["mx"], ref["mx"].float())
    exact("cam_excite.arg", t["arg"].cpu().to(torch.int64), ref["arg"])
    for k in ("avg", "ha", "hm", "gate"):
        check("cam_excite." + k, t[k], ref[k], unit[k])


def judge_bwd(t, ref, unit, B, Cn, Cr, init=None):
    ws = t["ws"].cpu()
    for k, part in (("du", ws[:B * Cn]), ("dta", ws[B * Cn:B * (Cn + Cr)]), ("dtm", ws[B * (Cn + Cr):])):
        check("cam_bwd." + k, part, ref[k], unit[k])
    check("cam_bwd.coefB", t["coefB"], ref["coefB"], unit["coefB"])
    check("cam_bwd.dmax", t["dmax"], ref["dmax"], unit["dmax"])
    for k, dk in (("dW1", "dw1"), ("dW2", "dw2")):
        r_, u_ = ref[k], unit[k]
        if init is not None:
            r_, u_ = r_ + init[dk].double(), u_ + init[dk].double().abs() + ref[k].abs()
        check("cam_bwd." + k, t[dk], r_, u_)


@pytest.mark.parametrize("name", list(CAM_MLP_CASES))
def test_cam_excite_on_planted_slabs(dev, name):
    from insar_unet_ca_amd._lib import call, stream_ptr
    c = cam_mlp_case(name)
    B, Cn, Cr = c["B"], c["C"], c["Cr"]
    ref, unit = cam_excite_ref(c)
    assert float(torch.cat([ref["pre_a"], ref["pre_m"]]).abs().min()) >= c["margin"] > 0
    ins = {k: c[k].to(dev) for k in ("psum", "pmax", "parg", "w1", "w2")}
    t = cam_out_buffers(dev, B, Cn, Cr)
    outs = ("avg", "mx", "arg", "ha", "hm", "gate")

    def prep():
        for k in outs:
            t[k].fill_(-7 if k == "arg" else float("nan"))
    before = {k: v.clone() for k, v in {**ins, **t}.items()}
    d = cam_desc(dev, B, c["H"], c["W"], Cn, Cr, c["rows"], {**t, **ins})
    twice(prep, lambda: call("insar_cam_excite", C.byref(d), stream_ptr()), [lambda k=k: t[k] for k in outs])
    untouched(before, {**ins, **t}, skip=outs)
    judge_excite(t, ref, unit)


@pytest.mark.parametrize("name", list(CAM_MLP_CASES))
def test_cam_bwd_coef_on_planted_inputs(dev, name):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    c = cam_mlp_case(name)
    B, Cn, Cr, acc = c["B"], c["C"], c["Cr"], c["acc"]
    ref, unit = cam_bwd_ref(c)
    ins = {k: c[k].to(dev) for k in ("w1", "w2", "gate", "ha", "hm", "avg", "mx")}
    red = c["red"].to(dev)
    t = cam_out_buffers(dev, B, Cn, Cr)
    t.update(ins)
    outs = ("ws", "coefB", "dmax", "dw1", "dw2")

    def prep():
        for k in ("ws", "coefB", "dmax"):
            t[k].fill_(float("nan"))
        for k in ("dw1", "dw2"):
            t[k].copy_(c[k + "_0"]) if acc else t[k].fill_(float("nan"))
    before = {k: v.clone() for k, v in t.items()}
    d = cam_desc(dev, B, c["H"], c["W"], Cn, Cr, 1, t, accumulate=acc)
    twice(prep, lambda: call("insar_cam_bwd_coef", C.byref(d), ptr(red), c["rows"], stream_ptr()), [lambda k=k: t[k] for k in outs])
    untouched(before, t, skip=outs)
    assert same(red, c["red"])
    judge_bwd(t, ref, unit, B, Cn, Cr, dict(dw1=c["dw1_0"], dw2=c["dw2_0"]) if acc else None)


def scatter_case(T):
    B, H, W, Cn = 2, 3, 5, 16
    g = _gen("scatter" + str(T))
    dx = torch.randn(B, H, W, Cn, generator=g).to(T)
    dmax = torch.randn(B, Cn, generator=g)
    arg = torch.randint(0, H * W, (B, Cn), generator=g)
    arg[:, 0], arg[:, 1], arg[:, 2], arg[:, 3] = 0, H * W - 1, 7, 7       # first pixel, last pixel, two channels on one pixel
    arg[1, 4], arg[1, 5] = H * W - 1, 0
    return dx, dmax, arg.to(torch.int32)


@pytest.mark.parametrize("sl", [None, (32, 0), (32, 16)], ids=["whole", "slice0of32", "slice16of32"])
@pytest.mark.parametrize("T", [F32, BF16], ids=["fp32", "bf16"])
def test_cam_scatter_max_is_exact(dev, T, sl):
    """round_T(float(old) + dmax) at the one target element of each (image, channel); every other element of the buffer,
    halo and neighbouring slice included, bitwise as it was."""
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    dx, dmax, arg = scatter_case(T)
    want, _ = A.cam_scatter_max(dx, dmax, arg, T)
    assert int((bits(want) != bits(dx)).sum()) <= dx.shape[0] * dx.shape[3]
    dm, ar = dmax.to(dev), arg.to(dev)
    seen = []
    for _ in range(2):
        a = upload(dev, dx, *(sl or ()))
        call("insar_cam_scatter_max", a.ref, ptr(dm), ptr(ar), stream_ptr())
        torch.cuda.synchronize()
        assert same(interior(a), want) and outside_untouched(a)
        seen.append(bits(a.buf))
    assert torch.equal(*seen) and same(dm, dmax) and same(ar, arg)


# --------------------------------------------------------------------------------------------------- CAM, chained
@pytest.mark.parametrize("T,shape,rpp,seed", [(BF16, (2, 7, 40, 64), 2, 2), (F32, (3, 5, 6, 256), 3, 6)],
                         ids=["bf16-2x7x40x64-rpp2", "fp32-3x5x6x256-rpp3"])
def test_cam_chain_each_launch_on_what_the_previous_one_wrote(dev, T, shape, rpp, seed):
    """pool -> excite -> (reduce) -> bwd_coef -> (apply) -> scatter_max: each CAM launch judged on the device's own tensors;
    the two BatchNorm-chain launches in brackets are plumbing here (tests/test_bn_backward_chain_gpu.py judges them). The
    seed was chosen so that the hidden pre-activations clear the ReLU margin (asserted below)."""
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    B, H, W, Cn = shape
    Cr, P = Cn // 16, -(-H // rpp)
    g = _gen(f"camchain{T}{shape}{seed}")
    x = (torch.randn(B, H, W, Cn, generator=g) + 0.3).to(T)
    dout = torch.randn(B, H, W, Cn, generator=g).to(T)
    w1, w2 = torch.randn(Cr, Cn, generator=g) / math.sqrt(Cn), torch.randn(Cn, Cr, generator=g) * 2 / math.sqrt(Cr)
    c = dict(T=T, B=B, H=H, W=W, C=Cn, rpp=rpp, P=P, x=x)
    xa, ga = upload(dev, x), upload(dev, dout)
    o = run_cam_pool(dev, c, xa)
    ref, unit = A.cam_pool(x, rpp)
    exact("cam_pool.pmax", o["pmax"], ref["pmax"].float())
    exact("cam_pool.parg", o["parg"].cpu().to(torch.int64), ref["parg"])
    check("cam_pool.psum", o["psum"], ref["psum"], unit["psum"])
    t = cam_out_buffers(dev, B, Cn, Cr)
    t.update(psum=o["psum"], pmax=o["pmax"], parg=o["parg"], w1=w1.to(dev), w2=w2.to(dev))
    d = cam_desc(dev, B, H, W, Cn, Cr, P, t)
    call("insar_cam_excite", C.byref(d), stream_ptr())
    torch.cuda.synchronize()
    ref, unit = A.cam_excite(o["psum"].cpu(), o["pmax"].cpu(), o["parg"].cpu(), w1, w2, H, W)
    pre = torch.cat([ref["pre_a"], ref["pre_m"]])
    assert float(pre.abs().min()) >= 1e-3 * float(pre.abs().max()) > 0          # on the slabs the device wrote
    assert bool((pre > 0).any()) and bool((pre < 0).any())
    judge_excite(t, ref, unit)
    ha, hm = t["ha"].cpu(), t["hm"].cpu()
    for h in (ha, hm):                                                          # and on the stored activations bwd_coef reads
        assert bool((h > 0).any()) and float(h[h > 0].min()) >= 1e-3 * float(h.max())
    one, zero = torch.ones(Cn, device=dev), torch.zeros(Cn, device=dev)
    red = nan_buf(dev, B, P, 2, Cn)
    call("insar_bnrelu_bwd_reduce", ga.ref, xa.ref, ptr(one), ptr(zero), ptr(red), 0, rpp, stream_ptr())
    call("insar_cam_bwd_coef", C.byref(d), ptr(red), P, stream_ptr())
    torch.cuda.synchronize()
    cpu = lambda k: t[k].cpu()
    ref, unit = A.cam_bwd_coef(red.cpu(), cpu("gate"), ha, hm, cpu("avg"), cpu("mx"), w1, w2, H, W)
    judge_bwd(t, ref, unit, B, Cn, Cr)
    dxa = upload(dev, torch.zeros(B, H, W, Cn, dtype=T))
    call("insar_bnrelu_bwd_apply", ga.ref, xa.ref, ptr(one), ptr(zero), ptr(zero), ptr(one), ptr(t["gate"]), ptr(t["coefB"]), ptr(zero),
         ptr(zero), dxa.ref, 0, stream_ptr())
    torch.cuda.synchronize()
    old = interior(dxa)
    call("insar_cam_scatter_max", dxa.ref, ptr(t["dmax"]), ptr(t["arg"]), stream_ptr())
    torch.cuda.synchronize()
    want, _ = A.cam_scatter_max(old, cpu("dmax"), cpu("arg"), T)
    assert same(interior(dxa), want) and outside_untouched(dxa)
    m, a = A._first_max(x.double().reshape(B, H * W, Cn), 1)
    exact("cam.mx of x", t["mx"], m.float())
    exact("cam.arg of x", cpu("arg").to(torch.int64), a)


# --------------------------------------------------------------------------------------------------- the float32 floor
def floor_ratios():
    """The float32-in-naive-order floor of every planted case against float64, per output: {name: ratio} (CPU only; fixes K)."""
    out = {}

    def fold(tag, ref, unit, lo):
        if isinstance(ref, dict):
            for k in ref:
                if ref[k] is not None and k not in ("arg", "parg", "pre_a", "pre_m"):
                    fold(f"{tag}.{k}", ref[k], unit[k], lo[k])
        else:
            out[tag] = max(out.get(tag, 0.0), R.ratio(lo, ref, unit))
    for name, launch in SA_PARAMS:
        c = sa_case(name)
        fold("sa_" + launch, *sa_ref(c, launch), sa_ref(c, launch, F32)[0])
    for name in CAM_POOL_CASES:
        c = cam_pool_case(name)
        fold("cam_pool", *A.cam_pool(c["x"], c["rpp"]), A.cam_pool(c["x"], c["rpp"], F32)[0])
    for name in CAM_MLP_CASES:
        c = cam_mlp_case(name)
        fold("cam_excite", *cam_excite_ref(c), cam_excite_ref(c, F32)[0])
        fold("cam_bwd", *cam_bwd_ref(c), cam_bwd_ref(c, F32)[0])
    return out
