"""GPU: the forward BatchNorm-apply family, MaxPool2d(2), the column sums and the two scalings of csrc/pointwise.hip, and
insar_se_res_apply (csrc/se_residual.hip), one launch at a time against the float64 reference tests/pointwise_ref.py.

Conventions of tests/test_bn_backward_chain_gpu.py: C entry points through _lib.call on planted stored operands; ReLU
pre-activations at least 1e-3 of the tensor's maximum away from 0 (enforce_margin), no element excluded; outputs pre-filled
with NaN, every other byte of a buffer (halo ring, neighbouring channels of a slice) with a sentinel that must survive;
every launch runs twice and must repeat itself bit for bit.

Tolerance, one rule: |got - ref| <= K * 2^-24 * U (U from the reference, an element with U = 0 exactly); a bf16 output may be
half a bf16 ulp of the reference further off. Exact outputs (pool values, arg maps, pool routing, the two scalings) are
compared bit for bit. K was fixed on the CPU before any kernel ran (tests/test_pointwise_ref_host.py):
    largest float32 floor ratio per output (the host file asserts each, rounded up to the next 0.01)
        apply 0.79  outc 0.54  bn_add_relu 0.68  se_res_apply 0.67  sum_hw 0.45  broadcast_hw 0.77  colsum 0.62
        colsum_partial 0.85  stem 0.58  stem_stats 1.01  stem_wgrad 0.91
    K = max(2 * 1.01, 2.76) = 2.76
Kernel, measured on an MI355X (largest ratio per output over all cases of this file):
        apply 0.78  apply_pool 0.70  apply_pool_arg 0.70  outc 0.53  se_res_apply 0.67  colsum 0.16  colsum_partial 0.70
    nothing needed more than 0.78 of the 2.76 allowed; every exact output matched bit for bit.

Work-group geometry (PW_THREADS = SER_THREADS = 256; a 16-byte chunk is 4 fp32 / 8 bf16 channels; cpp = C / chunk chunks per
pixel; wstep = 256 / cpp pixels per pass: C = 64 gives wstep 16 in fp32 and 32 in bf16; PW_UNROLL = 4; insar_grid_cap = 8192 rows):

  entry point                  path                                                       cases
  insar_bn_relu_apply          hoisted body (256 % cpp == 0), W <, ==, > wstep            apply: w15 w16 w17 w31 w32 w33
                               predicated tail of the 4 unrolled loads (W = 1, 4*wstep+1)  apply: w1 w65 w129
                               generic body (C = 96: cpp = 24 / 12 does not divide 256)    apply: c96 c96-nogate
                               cpp = 64 / 32, gate null / non-null, relu 0 / 1             apply: c256 and the (gate, relu) column
                               B*H = 8200 > 8192: a work-group serves image 0, then 1     apply: rows8200 (one gate negative)
                               dst (and y) a slice at channel 64 of a wider buffer         every apply case with B = 2, H < 100
  insar_bn_relu_apply_pool     W/2 <, ==, > wstep, cpp 16 / 8 / 64 / 32, pooled a slice    pool: p2 p30 p32 p34 p66 p128
  insar_bn_relu_apply_pool_arg the same + arg; both with B*H/2 = 8200                      pool: all, rows8200
                               ties at every pair of positions, ReLU zeros, NaN at each    pool_arg_events (fp32, bf16)
                               position, bf16 values 3/8 ulp apart before the store
  insar_bn_relu_apply_outc     K 1..4 (KM = 2 and 4), bias null / non-null                 outc: k1 k2 k3 k4
                               cpp = 1 (bf16 C=8), 2, 8, 16, 32, 64 (bf16 C=512)           outc: c8 c256 c512 (fp32 C=512 is refused)
                               W no multiple of wstep (idle lanes shuffle, never write)    outc: k1..k4 c8 w1; rows8200: gate reload
  insar_maxpool2_fwd / _bwd    odd H and W, ties, NaN, accumulate 0 / 1, refusal           maxpool2
  insar_colsum / _ld           rows 1 255 256 257 300 1000, tmp null, nsplit > 512, ld > cols   colsum: every COLSUM_CASES id; colsum_ws
  insar_colsum_partial         rps 1 / 7 / 128, ragged last split                          colsum_partial
  insar_scale_f32, insar_mul_dev_f32   n in 1 3 4 5 1023 1025, alignment                  scalings
  insar_se_res_apply           cpp < / >= 256, B*H > 8192 with a negative gate            se_res_apply
  every one                    INSAR_FAIL conditions of the host wrappers                  refusals

Kernel change this file forced: `pool_arg_events` — insar_bn_relu_apply_pool took the window maximum with fmaxf over the
unrounded values, which drops a NaN (the arg map and insar_maxpool2_fwd keep it) and prefers +0 to an earlier -0; it now
takes it over the stored values under insar_maxpool2_fwd's rule. Nothing else changed.
Wall time of the file on an MI355X: 2 s for its 124 tests (the slowest, 0.3 s, is the first launch).

The deeplab.hip half of the reference is held by tests/test_trunk_pointwise_gpu.py."""
import ctypes as C

import pytest
import torch

from tests import pointwise_cases as PC
from tests import pointwise_ref as R
from tests.pointwise_cases import BF16, F32, F64, tname
from tests.test_bn_backward_chain_gpu import SENTINEL, enforce_margin, interior, nan_buf, outside_untouched, upload

pytestmark = pytest.mark.gpu

K = 2.76
MEASURED = {}
E_SHAPE, E_DTYPE, E_ALIGN, E_WS, E_ARG = -1001, -1002, -1003, -1004, -1005


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


def out_act(dev, shape, T, Ctot=None, c_off=0):
    """An output slice: NaN inside, the sentinel everywhere else."""
    return upload(dev, torch.full(shape, float("nan"), dtype=T), Ctot, c_off)


def twice(run):
    """Run a launch twice on fresh outputs; both results must agree bit for bit. Returns the first."""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert R.bits_equal(x, y)
    return a


def sliced(shape):
    return (shape[3] + 128, 64) if shape[0] == 2 and shape[1] < 100 else (None, 0)


def refused(code, who, name, *args):
    """The call returns `code`, and insar_last_error names the entry point."""
    from insar_unet_ca_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    assert rc == code, (name, rc)
    assert who in lib.insar_last_error().decode()


IDS = lambda table: [f"{n}-{t}" for n in table for t in PC.DTYPES]
PAIRS = lambda table: [(n, T) for n in table for T in PC.DTYPES.values()]


# ------------------------------------------------------------------------------------------------ insar_bn_relu_apply
@pytest.mark.parametrize("name,T", PAIRS(PC.APPLY_SHAPES), ids=IDS(PC.APPLY_SHAPES))
def test_apply(dev, name, T):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    shape = PC.APPLY_SHAPES[name]
    c = PC.apply_case(shape, T, seed=2000 + sum(map(ord, name)))
    cpp = shape[3] // (8 if T == BF16 else 4)
    assert (256 % cpp == 0) == (shape[3] != 96)                                 # which body of bn_relu_apply_kernel this shape runs
    ya = upload(dev, c["y"], *sliced(shape))
    sc, sh, gt = c["scale"].to(dev), c["shift"].to(dev), c["gate"].to(dev) if c["gate"] is not None else None

    def run():
        da = out_act(dev, c["y"].shape, T, *sliced(shape))
        call("insar_bn_relu_apply", ya.ref, ptr(sc), ptr(sh), ptr(gt), da.ref, c["relu"], stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(da) and outside_untouched(ya)
        return (interior(da),)
    z, = twice(run)
    assert torch.equal(interior(ya), c["y"])
    check("apply", z, *R.bn_apply(c["y"], c["scale"], c["shift"], c["gate"], c["relu"]), T == BF16)


def run_pool(dev, c, T, with_arg, slices):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    B, H, W, Cn = c["y"].shape
    ya = upload(dev, c["y"])
    sc, sh, gt = c["scale"].to(dev), c["shift"].to(dev), c["gate"].to(dev) if c["gate"] is not None else None

    def run():
        da = out_act(dev, (B, H, W, Cn), T, *slices)
        pa = out_act(dev, (B, H // 2, W // 2, Cn), T, *slices)
        arg = torch.full((B, H // 2, W // 2, Cn), 9, dtype=torch.uint8, device=dev)
        if with_arg:
            call("insar_bn_relu_apply_pool_arg", ya.ref, ptr(sc), ptr(sh), ptr(gt), da.ref, pa.ref, ptr(arg), c["relu"], stream_ptr())
        else:
            call("insar_bn_relu_apply_pool", ya.ref, ptr(sc), ptr(sh), ptr(gt), da.ref, pa.ref, c["relu"], stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(da) and outside_untouched(pa) and outside_untouched(ya)
        return interior(da), interior(pa), arg.cpu()
    z, p, arg = twice(run)
    v, a = R.maxpool2(z)
    assert R.bits_equal(p, v)                                                   # the 2x2 maximum of the STORED dst
    assert torch.equal(arg, a if with_arg else torch.full_like(a, 9))
    return z


@pytest.mark.parametrize("name,T", PAIRS(PC.POOL_SHAPES), ids=IDS(PC.POOL_SHAPES))
def test_apply_pool(dev, name, T):
    shape = PC.POOL_SHAPES[name]
    c = PC.apply_case(shape, T, seed=2000 + sum(map(ord, name)))
    ref = R.bn_apply(c["y"], c["scale"], c["shift"], c["gate"], c["relu"])
    check("apply_pool_arg", run_pool(dev, c, T, True, sliced(shape)), *ref, T == BF16)
    check("apply_pool", run_pool(dev, c, T, False, sliced(shape)), *ref, T == BF16)


@pytest.mark.parametrize("T", [F32, BF16], ids=tname)
def test_pool_arg_events(dev, T):
    """Exact ties (equal positive values at every pair of positions and at all four, ReLU zeros), a NaN at each position,
    and (bf16) two values that differ before the store and are equal after it. The NaNs run with relu = 0: the kernels' ReLU
    is fmaxf(a, 0), which stores a NaN pre-activation as 0 (asserted here too), so only the no-ReLU form can store one."""
    c = PC.apply_case((1, 4, 16, 64, 1, 1), T, seed=41)
    c["gate"][0, 5], c["gate"][0, 3] = 0.5, 1.0
    y, c["scale"], c["shift"] = PC.plant_window_events(c["y"], c["scale"], c["shift"], T)
    y, _ = enforce_margin(y, c["scale"], c["shift"], T)
    c["y"] = PC.plant_nans(y)
    nan = torch.isnan(c["y"].float())
    clean = torch.where(nan, torch.ones_like(c["y"]), c["y"])
    for relu in (1, 0):
        c["relu"] = relu
        z = run_pool(dev, c, T, True, (None, 0))
        assert R.bits_equal(run_pool(dev, c, T, False, (None, 0)), z)
        zn = torch.isnan(z.float())
        assert int(nan.sum()) == 32 and (torch.equal(zn, nan) if not relu else (not bool(zn.any()) and bool((z[nan] == 0).all())))
        ref, u = R.bn_apply(clean, c["scale"], c["shift"], c["gate"], relu)
        check("apply_pool_arg", torch.where(nan, ref.to(T), z), ref, u, T == BF16)
        v, a = R.maxpool2(z)
        win = R._windows2(z).float()
        assert bool(((win == win.max(0).values).sum(0) > 1).any())
        if not relu:                                                            # a NaN wins its window, in the value and in the arg map
            assert int(torch.isnan(v.float()).sum()) == 32 and sorted(set(a[torch.isnan(v.float())].tolist())) == [0, 1, 2, 3]
        if T == BF16:                                                           # channel 3 of window 8: stored equal, arg = the first
            assert z[0, 2, 0, 3] == z[0, 3, 0, 3] == 3.75 and a[0, 1, 0, 3] == 0


# ------------------------------------------------------------------------------------------- insar_bn_relu_apply_outc
@pytest.mark.parametrize("name,T", PAIRS(PC.OUTC_SHAPES), ids=IDS(PC.OUTC_SHAPES))
def test_apply_outc(dev, name, T):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    c = PC.outc_case(name, T)
    B, H, W, Cn = c["y"].shape
    ya = upload(dev, c["y"])
    sc, sh, gt, w = c["scale"].to(dev), c["shift"].to(dev), c["gate"].to(dev) if c["gate"] is not None else None, c["wout"].to(dev)
    bias = c["bias"].to(dev) if c["bias"] is not None else None
    if Cn // (8 if T == BF16 else 4) > 64:
        lg = nan_buf(dev, B, c["K"], H, W)
        refused(E_SHAPE, "insar_bn_relu_apply_outc", "insar_bn_relu_apply_outc", ya.ref, ptr(sc), ptr(sh), ptr(gt), ptr(w), ptr(bias), ptr(lg), c["K"], c["relu"], stream_ptr())
        assert bool(torch.isnan(lg).all())
        return

    def run():
        lg = torch.full((B * c["K"] * H * W + 4,), float("nan"), device=dev)
        lg[-4:] = SENTINEL
        call("insar_bn_relu_apply_outc", ya.ref, ptr(sc), ptr(sh), ptr(gt), ptr(w), ptr(bias), ptr(lg), c["K"], c["relu"], stream_ptr())
        torch.cuda.synchronize()
        assert bool((lg[-4:] == SENTINEL).all()) and outside_untouched(ya)
        return (lg[:-4].view(B, c["K"], H, W).cpu(),)
    lg, = twice(run)
    check("outc", lg, *R.bn_apply_outc(c["y"], c["scale"], c["shift"], c["gate"], c["relu"], c["wout"], c["bias"], T))


# ------------------------------------------------------------------------------------------------ insar_maxpool2_*
@pytest.mark.parametrize("T", [F32, BF16], ids=tname)
@pytest.mark.parametrize("hw", [(7, 9), (4, 6), (2, 3), (9, 34)])
def test_maxpool2(dev, hw, T):
    """Forward values exact; backward exact against the reference routing (tests/test_pointwise_ref_host.py pins it to the
    autograd adjoint): an odd last row / column belongs to no window and is left as it was; accumulate = 0 on an odd grid is
    refused."""
    from insar_unet_ca_amd._lib import call, stream_ptr
    H, W = hw
    x = PC.rand_act((2, H, W, 64), T, 60 + H)
    x[:, 0:2, 0:2, :] = 0.5                                                     # all four equal
    x[1, 0, 1, 8:16], x[1, 1, 0, 16:24] = float("nan"), float("nan")
    x[0, 1, 1, :], x[0, 0, 0, 32:] = 3.0, 3.0                                   # (0,0) == (1,1) in half the channels
    dy, dx0 = PC.rand_act((2, H // 2, W // 2, 64), T, 61), PC.rand_act((2, H, W, 64), T, 62)
    xa, ga = upload(dev, x, 192, 64), upload(dev, dy)

    def fwd():
        pa = out_act(dev, tuple(dy.shape), T, 192, 64)
        call("insar_maxpool2_fwd", xa.ref, pa.ref, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(pa) and outside_untouched(xa)
        return (interior(pa),)
    assert R.bits_equal(twice(fwd)[0], R.maxpool2(x)[0])
    for acc in (1, 0):
        def bwd():
            da = upload(dev, dx0 if acc else torch.full_like(dx0, float("nan")), 192, 64)
            args = (xa.ref, ga.ref, da.ref, acc, stream_ptr())
            if not acc and (H | W) & 1:
                refused(E_SHAPE, "insar_maxpool2_bwd", "insar_maxpool2_bwd", *args)
                return (interior(da),)
            call("insar_maxpool2_bwd", *args)
            torch.cuda.synchronize()
            assert outside_untouched(da)
            return (interior(da),)
        dx, = twice(bwd)
        if not acc and (H | W) & 1:
            assert bool(torch.isnan(dx.float()).all())
        else:
            assert R.bits_equal(dx, R.maxpool2_bwd(x, dy, dx0, acc, T).to(T))


# ----------------------------------------------------------------------------------------------------- insar_colsum*
def colsum_tmp_floats(rows, seg, cols):
    rps = 128
    while -(-rows // rps) > 512:
        rps *= 2
    return -(-rows // rps) * seg * cols


@pytest.mark.parametrize("name", list(PC.COLSUM_CASES))
def test_colsum(dev, name):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    c = PC.colsum_case(name)
    seg, rows, cols, ld = c["seg"], c["rows"], c["cols"], c["ld"]
    buf = torch.full((seg, rows, ld), SENTINEL)
    buf[:, :, :cols] = c["part"]
    part = buf.to(dev)
    need = colsum_tmp_floats(rows, seg, cols)
    if name == "r65600":
        assert need == 257 * 3                                                  # nsplit = 513 at rps = 128: rps doubles

    def run():
        out = torch.full((seg * cols + 4,), SENTINEL, device=dev)
        out[:seg * cols] = c["out0"].reshape(-1).to(dev) if c["acc"] else float("nan")
        tmp = torch.full((need + 4,), SENTINEL, device=dev) if c["tmp"] else None
        if ld == cols:
            call("insar_colsum", ptr(part), ptr(out), seg, rows, cols, c["acc"], ptr(tmp), need, stream_ptr())
        else:
            call("insar_colsum_ld", ptr(part), ptr(out), seg, rows, cols, ld, c["acc"], ptr(tmp), need, stream_ptr())
        torch.cuda.synchronize()
        assert bool((out[-4:] == SENTINEL).all()) and (tmp is None or bool((tmp[need:] == SENTINEL).all()))
        return (out[:seg * cols].view(seg, cols).cpu(),)
    got, = twice(run)
    check("colsum", got, *R.colsum(c["part"], c["acc"], c["out0"]))
    assert torch.equal(part.cpu(), buf)


def test_colsum_workspace_one_short(dev):
    from insar_unet_ca_amd._lib import ptr, stream_ptr
    part = torch.randn(3, 300, 64, device=dev)
    out, tmp = nan_buf(dev, 3, 64), nan_buf(dev, 3 * 3 * 64)
    need = colsum_tmp_floats(300, 3, 64)
    assert need == tmp.numel()
    refused(E_WS, "insar_colsum", "insar_colsum", ptr(part), ptr(out), 3, 300, 64, 0, ptr(tmp), need - 1, stream_ptr())
    refused(E_WS, "insar_colsum_ld", "insar_colsum_ld", ptr(part), ptr(out), 3, 300, 32, 64, 0, ptr(tmp), need // 2 - 1, stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(tmp).all())


@pytest.mark.parametrize("name", list(PC.PARTIAL_CASES))
def test_colsum_partial(dev, name):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    rows, cols, rps = PC.PARTIAL_CASES[name]
    p = torch.randn(rows, cols, generator=PC.gen(rows))
    part, ns = p.to(dev), -(-rows // rps)

    def run():
        out = torch.full((ns * cols + 4,), float("nan"), device=dev)
        out[-4:] = SENTINEL
        call("insar_colsum_partial", ptr(part), ptr(out), rows, cols, rps, stream_ptr())
        torch.cuda.synchronize()
        assert bool((out[-4:] == SENTINEL).all())
        return (out[:-4].view(ns, cols).cpu(),)
    check("colsum_partial", twice(run)[0], *R.colsum_partial(p, rps))


# ------------------------------------------------------------------------------ insar_scale_f32, insar_mul_dev_f32
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025])
def test_scalings(dev, n):
    """One fp32 multiply each: torch's fp32 product, bit for bit; the element behind the last stays. insar_mul_dev_f32
    wants 16-byte-aligned out and x (any n: the n % 4 tail goes element by element) and refuses anything else."""
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    x = torch.randn(n, generator=PC.gen(n))
    s = torch.tensor([0.3], dtype=F32)
    want = x * s
    s_d = s.to(dev)

    def run():
        p = torch.full((n + 1,), SENTINEL, device=dev)
        p[:n] = x.to(dev)
        call("insar_scale_f32", ptr(p), n, 0.3, stream_ptr())
        xin = torch.full((n + 4,), SENTINEL, device=dev)
        xin[:n] = x.to(dev)
        out = torch.full((n + 4,), SENTINEL, device=dev)
        out[:n] = float("nan")
        call("insar_mul_dev_f32", ptr(out), ptr(xin), n, ptr(s_d), stream_ptr())
        torch.cuda.synchronize()
        assert p[n] == SENTINEL and bool((out[n:] == SENTINEL).all()) and torch.equal(xin[:n].cpu(), x)
        return p[:n].cpu(), out[:n].cpu()
    a, b = twice(run)
    assert R.bits_equal(a, want) and R.bits_equal(b, want)
    buf = nan_buf(dev, n + 8)
    for o, i in ((buf[1:], buf[4:]), (buf[4:], buf[1:])):                       # a 4-byte offset of either operand
        refused(E_ALIGN, "insar_mul_dev_f32", "insar_mul_dev_f32", ptr(o), ptr(i), n, ptr(s_d), stream_ptr())
    refused(E_ARG, "insar_mul_dev_f32", "insar_mul_dev_f32", ptr(buf), 0, n, ptr(s_d), stream_ptr())
    refused(E_ARG, "insar_scale_f32", "insar_scale_f32", 0, n, 0.3, stream_ptr())
    call("insar_mul_dev_f32", ptr(buf), ptr(buf), 0, ptr(s_d), stream_ptr())     # n = 0: accepted, nothing launched
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ------------------------------------------------------------------------------------------------ insar_se_res_apply
SE_RES_SHAPES = {"c64": (2, 3, 7, 64), "c256": (2, 2, 33, 256), "c2048": (1, 2, 3, 2048), "rows8200": (2, 4100, 2, 64)}


@pytest.mark.parametrize("name,T", PAIRS(SE_RES_SHAPES), ids=IDS(SE_RES_SHAPES))
def test_se_res_apply(dev, name, T):
    from insar_unet_ca_amd._lib import call, ptr, stream_ptr
    B, H, W, Cn = shape = SE_RES_SHAPES[name]
    c = PC.apply_case(shape + (1, 1), T, seed=4000 + Cn + H)
    res = PC.rand_act(shape, T, 70)
    g = c["gate"][:, None, None, :]
    y, _ = enforce_margin(c["y"], g * c["scale"], g.double() * c["shift"].double() + res.double(), T)
    ya, ra = upload(dev, y, *sliced(shape)), upload(dev, res)
    sc, sh, gt = c["scale"].to(dev), c["shift"].to(dev), c["gate"].to(dev)

    def run():
        da = out_act(dev, shape, T, *sliced(shape))
        call("insar_se_res_apply", ya.ref, ptr(sc), ptr(sh), ptr(gt), ra.ref, da.ref, stream_ptr())
        torch.cuda.synchronize()
        assert outside_untouched(da) and outside_untouched(ya) and outside_untouched(ra)
        return (interior(da),)
    check("se_res_apply", twice(run)[0], *R.se_res_apply(y, c["scale"], c["shift"], c["gate"], res), T == BF16)


# ------------------------------------------------------------------------------------------------------- refusals
# each row: entry point, documented code, arguments built from the fixture x (x.y, x.d: 2x4x6x64 fp32 slices, x.p: their
# pooled grid, x.lg: logits, x.v: a device vector, x.mk(B, H, W, C, T): a fresh NaN-filled slice, x.s: the stream)
REFUSALS = [
    ("insar_bn_relu_apply", E_SHAPE, lambda x: (x.y.ref, x.v, x.v, 0, x.mk(2, 4, 5, 64).ref, 1, x.s)),
    ("insar_bn_relu_apply", E_SHAPE, lambda x: (x.y.ref, x.v, x.v, 0, x.mk(2, 4, 6, 64, BF16).ref, 1, x.s)),
    ("insar_bn_relu_apply", E_ARG, lambda x: (x.y.ref, 0, x.v, 0, x.d.ref, 1, x.s)),
    ("insar_bn_relu_apply", E_ARG, lambda x: (None, x.v, x.v, 0, x.d.ref, 1, x.s)),
    ("insar_bn_relu_apply", E_SHAPE, lambda x: (x.act(x.y.buf, 2, 4, 6, 64, 2, 60).ref, x.v, x.v, 0, x.d.ref, 1, x.s)),
    ("insar_bn_relu_apply_pool", E_SHAPE, lambda x: (x.mk(2, 5, 6, 64).ref, x.v, x.v, 0, x.mk(2, 5, 6, 64).ref, x.p.ref, 1, x.s)),
    ("insar_bn_relu_apply_pool", E_SHAPE, lambda x: (x.y.ref, x.v, x.v, 0, x.d.ref, x.mk(2, 2, 2, 64).ref, 1, x.s)),
    ("insar_bn_relu_apply_pool", E_SHAPE, lambda x: (x.mk(2, 4, 6, 96).ref, x.v, x.v, 0, x.mk(2, 4, 6, 96).ref, x.mk(2, 2, 3, 96).ref, 1, x.s)),
    ("insar_bn_relu_apply_pool", E_ARG, lambda x: (x.y.ref, x.v, 0, 0, x.d.ref, x.p.ref, 1, x.s)),
    ("insar_bn_relu_apply_pool_arg", E_ARG, lambda x: (x.y.ref, x.v, x.v, 0, x.d.ref, x.p.ref, 0, 1, x.s)),
    ("insar_bn_relu_apply_outc", E_SHAPE, lambda x: (x.y.ref, x.v, x.v, 0, x.v, 0, x.ptr(x.lg), 0, 1, x.s)),
    ("insar_bn_relu_apply_outc", E_SHAPE, lambda x: (x.y.ref, x.v, x.v, 0, x.v, 0, x.ptr(x.lg), 5, 1, x.s)),
    ("insar_bn_relu_apply_outc", E_SHAPE, lambda x: (x.mk(2, 4, 6, 96).ref, x.v, x.v, 0, x.v, 0, x.ptr(x.lg), 2, 1, x.s)),
    ("insar_bn_relu_apply_outc", E_ARG, lambda x: (x.y.ref, x.v, x.v, 0, x.v, 0, 0, 2, 1, x.s)),
    ("insar_bn_relu_apply_outc", E_ARG, lambda x: (x.y.ref, x.v, x.v, 0, 0, 0, x.ptr(x.lg), 2, 1, x.s)),
    ("insar_maxpool2_fwd", E_SHAPE, lambda x: (x.y.ref, x.mk(2, 2, 2, 64).ref, x.s)),
    ("insar_maxpool2_fwd", E_SHAPE, lambda x: (x.mk(2, 1, 6, 64).ref, x.mk(2, 1, 3, 64).ref, x.s)),
    ("insar_maxpool2_bwd", E_SHAPE, lambda x: (x.y.ref, x.p.ref, x.mk(2, 4, 6, 128).ref, 1, x.s)),
    ("insar_colsum", E_ARG, lambda x: (0, x.ptr(x.lg), 1, 4, 4, 0, 0, 0, x.s)),
    ("insar_colsum", E_SHAPE, lambda x: (x.v, x.ptr(x.lg), 0, 4, 4, 0, 0, 0, x.s)),
    ("insar_colsum_ld", E_SHAPE, lambda x: (x.v, x.ptr(x.lg), 1, 4, 4, 3, 0, 0, 0, x.s)),
    ("insar_colsum_partial", E_SHAPE, lambda x: (x.v, x.ptr(x.lg), 4, 4, 0, x.s)),
    ("insar_colsum_partial", E_SHAPE, lambda x: (x.v, x.ptr(x.lg), 65536, 4, 1, x.s)),
    ("insar_colsum_partial", E_ARG, lambda x: (x.v, 0, 4, 4, 1, x.s)),
    ("insar_se_res_apply", E_ARG, lambda x: (x.y.ref, x.v, x.v, 0, x.d.ref, x.d.ref, x.s)),
    ("insar_se_res_apply", E_SHAPE, lambda x: (x.y.ref, x.v, x.v, x.v, x.mk(2, 4, 5, 64).ref, x.d.ref, x.s)),
    ("insar_se_res_apply", E_SHAPE, lambda x: (x.mk(2, 4, 6, 96).ref, x.v, x.v, x.v, x.mk(2, 4, 6, 96).ref, x.mk(2, 4, 6, 96).ref, x.s)),
]


class RefusalFixture:
    """Operands of one refused call: every slice it hands out is NaN inside and is checked to stay so."""

    def __init__(self, dev):
        from insar_unet_ca_amd.engine import Act
        from insar_unet_ca_amd._lib import ptr, stream_ptr
        self.dev, self.act, self.ptr, self.s, self.made = dev, Act, ptr, stream_ptr(), []
        self.y, self.d, self.p = self.mk(2, 4, 6, 64), self.mk(2, 4, 6, 64), self.mk(2, 2, 3, 64)
        self.lg = nan_buf(dev, 2, 4, 4, 6)
        self.vec = torch.ones(512, device=dev)
        self.v = ptr(self.vec)

    def mk(self, B, H, W, Cn, T=F32):
        self.made.append(out_act(self.dev, (B, H, W, Cn), T))
        return self.made[-1]

    def untouched(self):
        torch.cuda.synchronize()
        return (all(bool(torch.isnan(interior(a).float()).all()) and outside_untouched(a) for a in self.made)
                and bool(torch.isnan(self.lg).all()) and bool((self.vec == 1).all()))


@pytest.mark.parametrize("i", range(len(REFUSALS)), ids=[f"{r[0]}-{i}" for i, r in enumerate(REFUSALS)])
def test_refusals(dev, i):
    """One INSAR_FAIL condition of a host wrapper: the documented code, insar_last_error names the entry point, nothing is
    launched (every output keeps its NaN pre-fill)."""
    name, code, build = REFUSALS[i]
    x = RefusalFixture(dev)
    refused(code, name.replace("_pool_arg", "_pool") if code == E_SHAPE else name, name, *build(x))
    assert x.untouched()


def test_print_measured():
    """Last in the file: the largest kernel ratio per output (visible with -s)."""
    print("MEASURED", "  ".join(f"{k} {v:.2f}" for k, v in sorted(MEASURED.items())))
