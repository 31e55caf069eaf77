"""CPU: tests/pointwise_ref.py against independent torch formulations (<= 1e-12), the float32 floor that fixes K for
tests/test_forward_apply_gpu.py and tests/test_trunk_pointwise_gpu.py, and the proof that the case tables can see the errors
they are there for: a float32 emulation of each kernel's formula with one mutation at a time must fall outside the
acceptance rule (the bound, or exactness) on at least one case.

K: twice the largest float32 floor ratio over all value outputs and all cases (FLOOR below, asserted here), but not below
the project's smallest existing K, 2.76 (tests/test_attention_units_gpu.py). FLOOR holds each measured floor rounded UP to
the next 0.01 (an upper bound that the test asserts); the largest is 1.01 (the stem's statistics rows), twice that is below
2.76, so K = 2.76."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_cases as PC
from tests import pointwise_ref as R
from tests.pointwise_cases import BF16, F32, F64

K = 2.76
# largest |f32 - f64| / (2^-24 * U) per value output over the case tables (float32 in naive order, on the CPU), rounded up
FLOOR = {"apply": 0.79, "outc": 0.54, "bn_add_relu": 0.68, "se_res_apply": 0.67, "sum_hw": 0.45, "broadcast_hw": 0.77,
         "colsum": 0.62, "colsum_partial": 0.85, "stem": 0.58, "stem_stats": 1.01, "stem_wgrad": 0.91}


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------ reference against torch
@pytest.mark.parametrize("name", ["w17", "w33", "c96", "c256"])
def test_apply_family_against_torch(name):
    c = PC.apply_case(PC.APPLY_SHAPES[name], F32, seed=1)
    y, sc, sh, relu = c["y"].double(), c["scale"].double(), c["shift"].double(), c["relu"]
    a = F.batch_norm(nchw(y), torch.zeros_like(sc), torch.ones_like(sc) - 1e-5, sc, sh, False, 0.0, 1e-5)
    z = F.relu(a) if relu else a
    if c["gate"] is not None:
        z = z * c["gate"].double()[:, :, None, None]
    assert rel(nchw(R.bn_apply(c["y"], c["scale"], c["shift"], c["gate"], relu)[0]), z) <= 1e-12
    res = PC.rand_act(tuple(c["y"].shape), F32, 5)
    assert rel(nchw(R.bn_add_relu(c["y"], c["scale"], c["shift"], res, 1)[0]), F.relu(a + nchw(res.double()))) <= 1e-12
    assert rel(nchw(R.bn_add_relu(c["y"], c["scale"], c["shift"], res, 0)[0]), a + nchw(res.double())) <= 1e-12
    gt = PC.gates(c["B"], c["C"], 3)
    want = F.relu(gt.double()[:, :, None, None] * a + nchw(res.double()))
    assert rel(nchw(R.se_res_apply(c["y"], c["scale"], c["shift"], gt, res)[0]), want) <= 1e-12
    for T in (F32, BF16):
        w, b = torch.randn(3, c["C"]), torch.randn(3)
        zr = R.stored(nhwc(z).contiguous(), T)
        want = F.conv2d(nchw(zr), w.double()[:, :, None, None], b.double())
        assert rel(R.bn_apply_outc(c["y"], c["scale"], c["shift"], c["gate"], relu, w, b, T)[0], want) <= 1e-12


@pytest.mark.parametrize("hw", [(4, 6), (7, 9), (8, 9), (1, 5), (5, 1), (9, 8)])
def test_pools_against_torch_and_autograd(hw):
    H, W = hw
    x = torch.randn(2, H, W, 8, generator=PC.gen(H * 10 + W), dtype=F64)
    xr = nchw(x).clone().requires_grad_(True)
    v, idx = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    got, arg = R.maxpool3s2(x)
    assert torch.equal(nchw(got), v.detach())
    ho, wo = torch.arange(v.shape[2])[:, None], torch.arange(v.shape[3])[None, :]
    want_arg = (idx // W - 2 * ho + 1) * 3 + (idx % W - 2 * wo + 1)
    assert torch.equal(nchw(arg).long(), want_arg)
    g = torch.randn(v.shape, generator=PC.gen(3), dtype=F64)
    v.backward(g)
    assert rel(nchw(R.maxpool3s2_bwd(nhwc(g), arg, H, W, F64, dt=F64)), xr.grad) <= 1e-12
    if H >= 2 and W >= 2:
        xr = nchw(x).clone().requires_grad_(True)
        v, idx = F.max_pool2d(xr, 2, return_indices=True)
        got, arg = R.maxpool2(x)
        assert torch.equal(nchw(got), v.detach())
        ho, wo = torch.arange(v.shape[2])[:, None], torch.arange(v.shape[3])[None, :]
        assert torch.equal(nchw(arg).long(), (idx // W - 2 * ho) * 2 + (idx % W - 2 * wo))
        g = torch.randn(v.shape, generator=PC.gen(4), dtype=F64)
        v.backward(g)
        dx0 = torch.randn(x.shape, generator=PC.gen(5), dtype=F64)
        assert rel(nchw(R.maxpool2_bwd(x, nhwc(g), dx0, 1, F64)), xr.grad + nchw(dx0)) <= 1e-12
        if not (H | W) & 1:
            assert rel(nchw(R.maxpool2_bwd(x, nhwc(g), dx0, 0, F64)), xr.grad) <= 1e-12


def test_pool_rules_on_ties_and_nan():
    """First maximum in scan order, NaN wins — torch's CPU max-pools decide the same way."""
    x = torch.zeros(1, 4, 4, 1)
    x[0, :2, :2, 0] = torch.tensor([[1.0, 2.0], [2.0, 0.0]])
    x[0, :2, 2:, 0] = torch.tensor([[1.0, float("nan")], [5.0, 0.0]])
    v, arg = R.maxpool2(x)
    assert arg[0, 0, :, 0].tolist() == [1, 1] and arg[0, 1, :, 0].tolist() == [0, 0] and bool(torch.isnan(v[0, 0, 1, 0]))
    tv, ti = F.max_pool2d(nchw(x), 2, return_indices=True)
    assert ti[0, 0, 0].tolist() == [1, 3] and R.maxpool2(x, last=True)[1][0, 0, 0, 0] == 2
    x3 = torch.full((1, 5, 5, 1), 0.5)
    v3, a3 = R.maxpool3s2(x3)
    assert a3[0, :, :, 0].tolist() == [[4, 3, 3], [1, 0, 0], [1, 0, 0]]        # clipped windows start at their first valid tap
    t3 = F.max_pool2d(nchw(x3), 3, 2, 1, return_indices=True)[1][0, 0]
    assert t3.tolist() == [[0, 1, 3], [5, 6, 8], [15, 16, 18]]
    x3[0, 2, 2, 0] = float("nan")
    assert R.maxpool3s2(x3)[1][0, 1, 1, 0] == 4 and R.maxpool3s2(torch.full((1, 3, 3, 1), -math.inf))[1][0, 0, 0, 0] == 4


@pytest.mark.parametrize("name", list(PC.STEM_CASES))
def test_stem_against_conv2d_and_autograd(name):
    for T, rep in ((F32, True), (BF16, True), (BF16, False)):
        c = PC.stem_case(name, T, rep)
        xr, w = R.stored(c["x"].double(), T)[:, None], R.stored(c["w"].double(), T).view(64, 1, 7, 7).requires_grad_(True)
        y = F.conv2d(xr, w, None, stride=2, padding=3)
        ref, u = R.conv7x7s2(c["x"], c["w"], T)
        assert rel(nchw(ref), y.detach()) <= 1e-12 and bool((u >= ref.abs()).all())
        st, _ = R.stem_stats(ref)
        assert rel(st[:, 0], nhwc(y.detach()).sum(2).reshape(-1, 64)) <= 1e-12 and rel(st[:, 1], (nhwc(y.detach()) ** 2).sum(2).reshape(-1, 64)) <= 1e-12
        part, _ = R.conv7x7s2_wgrad(c["x"], c["dy"], T)
        y.backward(nchw(c["dy"].double()))
        assert rel(part.sum(0), w.grad.reshape(-1)) <= 1e-12
        g0 = c["dy"].double().reshape(-1, c["W"] // 2, 64).clone()
        g0[8:] = 0                                                              # the first block alone: rows 0..7 across the images
        w.grad = None
        F.conv2d(xr, w, None, stride=2, padding=3).backward(nchw(g0.view(c["dy"].shape)))
        assert rel(part[0], w.grad.reshape(-1)) <= 1e-12


def test_sums_and_broadcast_against_torch():
    for name in PC.SUMHW_CASES:
        B, H, W, Cn, f = PC.SUMHW_CASES[name]
        x = PC.rand_act((B, H, W, Cn), BF16, 7)
        assert rel(R.sum_hw(x, f)[0], x.double().sum((1, 2)) * R.f32(f)) <= 1e-12
        src, d0 = torch.randn(B, Cn), PC.rand_act((B, H, W, Cn), BF16, 8)
        gate = PC.rand_act((B, H, W, Cn), BF16, 9)
        want = d0.double() + R.f32(f) * src.double()[:, None, None, :]
        assert rel(R.broadcast_hw(src, d0, f, 1)[0], want) <= 1e-12
        assert rel(R.broadcast_hw(src, d0, f, 1, gate)[0], want * (gate > 0)) <= 1e-12
    for name in PC.COLSUM_CASES:
        c = PC.colsum_case(name)
        assert rel(R.colsum(c["part"], 1, c["out0"])[0], c["part"].double().sum(1) + c["out0"].double()) <= 1e-12
    for name, (rows, cols, rps) in PC.PARTIAL_CASES.items():
        p = torch.randn(rows, cols, generator=PC.gen(rows))
        want = torch.stack([p[r:r + rps].double().sum(0) for r in range(0, rows, rps)])
        assert rel(R.colsum_partial(p, rps)[0], want) <= 1e-12


# --------------------------------------------------------------------------------------------------- the float32 floor
def floor_ratios():
    out = {}

    def put(name, fn, *a, **kw):
        ref, u = fn(*a, **kw)
        lo, _ = fn(*a, **kw, dt=F32)
        out[name] = max(out.get(name, 0.0), R.ratio(lo, ref, u))

    for T in (F32, BF16):
        for name, shape in list(PC.APPLY_SHAPES.items()) + list(PC.POOL_SHAPES.items()):
            c = PC.apply_case(shape, T, seed=2000 + sum(map(ord, name)))
            put("apply", R.bn_apply, c["y"], c["scale"], c["shift"], c["gate"], c["relu"])
            if shape[1] <= 100:
                res, gt = PC.rand_act(tuple(c["y"].shape), T, 11), PC.gates(c["B"], c["C"], 12)
                put("bn_add_relu", R.bn_add_relu, c["y"], c["scale"], c["shift"], res, c["relu"])
                put("se_res_apply", R.se_res_apply, c["y"], c["scale"], c["shift"], gt, res)
        for name in PC.OUTC_SHAPES:
            c = PC.outc_case(name, T)
            put("outc", R.bn_apply_outc, c["y"], c["scale"], c["shift"], c["gate"], c["relu"], c["wout"], c["bias"], T)
        for name, (B, H, W, Cn, f) in PC.SUMHW_CASES.items():
            x = PC.rand_act((B, H, W, Cn), T, 21)
            put("sum_hw", R.sum_hw, x, f)
            put("broadcast_hw", R.broadcast_hw, torch.randn(B, Cn, generator=PC.gen(22)), x, f, 1)
        for name in PC.STEM_CASES:
            for rep in (True, False):
                c = PC.stem_case(name, T, rep)
                put("stem", R.conv7x7s2, c["x"], c["w"], T)
                put("stem_stats", R.stem_stats, R.conv7x7s2(c["x"], c["w"], T)[0].float().to(T))
                put("stem_wgrad", R.conv7x7s2_wgrad, c["x"], c["dy"], T)
    for name in PC.COLSUM_CASES:
        c = PC.colsum_case(name)
        put("colsum", R.colsum, c["part"], c["acc"], c["out0"])
    for name, (rows, cols, rps) in PC.PARTIAL_CASES.items():
        put("colsum_partial", R.colsum_partial, torch.randn(rows, cols, generator=PC.gen(rows)), rps)
    return out


def test_float32_floor_fixes_k():
    got = floor_ratios()
    print("float32 floor:", "  ".join(f"{k} {v:.2f}" for k, v in got.items()))
    assert set(got) == set(FLOOR)
    for k, v in got.items():
        assert v <= FLOOR[k], (k, v)
    assert K == max(2.76, 2 * max(FLOOR.values()))


# ----------------------------------------------------------------------------------------------------- sensitivity
def rejected(got, ref, unit, bf16_out=False):
    return R.excess(got, ref, unit, K, bf16_out) > K


def gated_cases(T):
    for name, shape in PC.APPLY_SHAPES.items():
        if shape[4] and shape[1] <= 100:
            yield PC.apply_case(shape, T, seed=2000 + sum(map(ord, name)))


def test_apply_mutants_are_rejected():
    hits = {"gate of image n-1": 0, "relu after the gate": 0, "shift of channel c+1": 0, "bf16 store by truncation": 0, "none": 0}
    for T in (F32, BF16):
        for c in gated_cases(T):
            a = (c["y"], c["scale"], c["shift"])
            ref, u = R.bn_apply(*a, c["gate"], c["relu"])
            bf = T == BF16
            st = lambda v: v.to(T)
            hits["none"] += rejected(st(R.bn_apply(*a, c["gate"], c["relu"], dt=F32)[0]), ref, u, bf)
            hits["gate of image n-1"] += rejected(st(R.bn_apply(*a, c["gate"].roll(1, 0), c["relu"], dt=F32)[0]), ref, u, bf)
            hits["shift of channel c+1"] += rejected(st(R.bn_apply(c["y"], c["scale"], c["shift"].roll(-1), c["gate"], c["relu"], dt=F32)[0]), ref, u, bf)
            if c["relu"]:
                late = (c["y"].float() * c["scale"] + c["shift"]) * c["gate"][:, None, None, :]
                hits["relu after the gate"] += rejected(st(late.clamp_min(0)), ref, u, bf)
            if bf:
                hits["bf16 store by truncation"] += rejected(PC.trunc_bf16(R.bn_apply(*a, c["gate"], c["relu"], dt=F32)[0]), ref, u, True)
    assert hits.pop("none") == 0 and all(v > 0 for v in hits.values()), hits


def test_pool_mutants_are_rejected():
    c = PC.apply_case((1, 4, 16, 64, 0, 1), BF16, seed=41)
    y, sc, sh = PC.plant_window_events(c["y"], c["scale"], c["shift"], BF16)
    y, _ = PC.enforce_margin(y, sc, sh, BF16)
    z32 = R.bn_apply(y, sc, sh, None, 1, dt=F32)[0]
    z = z32.to(BF16)
    v, arg = R.maxpool2(z)
    assert not torch.equal(R.maxpool2(z, last=True)[1], arg)                    # tie resolved to the last maximum
    assert R.bits_equal(R.maxpool2(z, last=True)[0], v)                         # ... which only the arg map and the routing can see
    assert not torch.equal(R.maxpool2(z32)[1], arg)                             # arg from the unrounded values
    x = PC.rand_act((2, 7, 9, 64), BF16, 42)
    v3, a3 = R.maxpool3s2(x)
    vm, am = R.maxpool3s2(x, clamp_left=True)
    assert R.bits_equal(vm, v3) and not torch.equal(am, a3)                     # column -1 read as column 0: the arg map moves
    dy = PC.rand_act(tuple(v3.shape), BF16, 43)
    assert not R.bits_equal(R.maxpool3s2_bwd(dy, am, 7, 9, BF16).to(BF16), R.maxpool3s2_bwd(dy, a3, 7, 9, BF16).to(BF16))


def test_stem_and_colsum_mutants_are_rejected():
    hit_tap = hit_stats = 0
    for name in PC.STEM_CASES:
        c = PC.stem_case(name, BF16)
        ref, u = R.conv7x7s2(c["x"], c["w"], BF16)
        lo = R.conv7x7s2(c["x"], c["w"], BF16, dt=F32)[0]
        assert not rejected(lo.to(BF16), ref, u, True)
        mut = lo.clone()
        mut[:, :, 0, :] -= c["x"][:, 0::2, 0, None] * c["w"][None, None, :, 3 * 7 + 3]      # tap (3, 3) of the pixels wo = 0 dropped
        hit_tap += rejected(mut.to(BF16), ref, u, True)
        sref, su = R.stem_stats(lo.to(BF16))
        assert not rejected(R.stem_stats(lo.to(BF16), dt=F32)[0], sref, su)
        hit_stats += rejected(R.stem_stats(lo, dt=F32)[0], sref, su)            # statistics of the unrounded accumulator
    assert hit_tap == len(PC.STEM_CASES) and hit_stats > 0
    hit = 0
    for name in PC.COLSUM_CASES:
        c = PC.colsum_case(name)
        ref, u = R.colsum(c["part"], c["acc"], c["out0"])
        lo = R.colsum(c["part"], c["acc"], c["out0"], dt=F32)[0]
        assert not rejected(lo, ref, u)
        if 256 < c["rows"] <= 1000:     # (one row of 65 600 lies inside the bound of so long a sum: the shorter two-stage cases see it)
            hit += rejected(lo - c["part"][:, 128], ref, u)                     # the first row of the second split skipped
    assert hit == sum(1 for v in PC.COLSUM_CASES.values() if 256 < v[1] <= 1000) > 0


# ------------------------------------------------------------------------------------------------- bilinear resizes
# The resizes keep a K of their own, fixed the same way: the float32 floor of R.resize_fwd / R.resize_bwd over PC.RESIZE_CASES
# (rounded up), K_RESIZE = max(2.76, twice the largest). The floor is above 1 where src is not exact in float32: the weight of
# a tap then carries an absolute error of about 2^-24 * src, whatever its own size (shrinking 13 x 30 -> 5 x 7, the ragged
# up-samplings), and an output whose float32 src rounds to the other side of an integer takes the neighbouring index pair.
# Measured: forward 91.19 (24 x 46 -> 25 x 47, src up to 45), adjoint 110.52 (13 x 30 -> 5 x 7); 0 for equal sizes, at most 3.1
# where the scale is a power of two. The floor exceeds 1, so K_RESIZE = 2 * 110.52 (tests/pointwise_cases.py).
FLOOR_RESIZE, K_RESIZE = PC.RESIZE_FLOOR, PC.RESIZE_K


def test_resize_reference_against_interpolate_and_autograd():
    for name in PC.RESIZE_CASES:
        c = PC.resize_case(name, F32, Cn=8)
        xr = nchw(c["x"].double()).contiguous().requires_grad_(True)
        want = F.interpolate(xr, size=c["out"], mode="bilinear", align_corners=False)
        ref, u = R.resize_fwd(c["x"], c["out"])
        assert rel(ref, nhwc(want.detach())) <= 1e-12, name
        assert bool((u >= ref.abs() * (1 - 1e-12)).all())
        want.backward(nchw(c["g"].double()))
        dref, du = R.resize_bwd(c["g"], c["in"])
        assert rel(dref, nhwc(xr.grad)) <= 1e-12, name
        assert bool((du >= dref.abs() * (1 - 1e-12)).all())
        # <A x, g> = <x, A^T g>: the adjoint is the transpose of the forward's weights
        assert abs(float((ref * c["g"].double()).sum() - (c["x"].double() * dref).sum())) <= 1e-9
    c = PC.resize_case("same", BF16)
    assert R.bits_equal(R.resize_fwd(c["x"], c["out"])[0], c["x"].double())       # equal sizes: the identity
    assert R.bits_equal(R.resize_bwd(c["g"], c["in"])[0], c["g"].double())


def resize_floor():
    out = {"resize_fwd": {}, "resize_bwd": {}}
    for T in (F32, BF16):
        for name in PC.RESIZE_CASES:
            c = PC.resize_case(name, T, Cn=8)
            ref, u = R.resize_fwd(c["x"], c["out"])
            out["resize_fwd"][name, T] = R.ratio(R.resize_fwd(c["x"], c["out"], dt=F32)[0], ref, u)
            ref, u = R.resize_bwd(c["g"], c["in"])
            out["resize_bwd"][name, T] = R.ratio(R.resize_bwd(c["g"], c["in"], dt=F32)[0], ref, u)
    return out


def test_resize_float32_floor_fixes_k():
    got = resize_floor()
    for k, per_case in got.items():
        print(f"float32 floor {k}:", "  ".join(f"{n}-{PC.tname(T)} {v:.2f}" for (n, T), v in per_case.items()))
        assert max(per_case.values()) <= FLOOR_RESIZE[k], (k, max(per_case.values()))
    assert K_RESIZE == max(2.76, 2 * max(FLOOR_RESIZE.values()))
    for name in ("same",):                                       # exact cases: float32 gives the float64 result
        assert got["resize_fwd"][name, F32] == 0 and got["resize_bwd"][name, F32] == 0


def test_resize_mutants_are_rejected():
    hits = dict.fromkeys(R.RESIZE_PLANTS, 0)
    for T in (F32, BF16):
        for name in PC.RESIZE_CASES:
            c = PC.resize_case(name, T, Cn=8)
            ref, u = R.resize_fwd(c["x"], c["out"])
            dref, du = R.resize_bwd(c["g"], c["in"])
            assert not rejected_resize(ref, ref, u, T) and not rejected_resize(dref, dref, du, T)
            for plant in R.RESIZE_PLANTS:
                bad = R.resize_bwd(c["g"], c["in"], plant=plant)[0]
                hit = rejected_resize(bad, dref, du, T)
                if plant != "window_short":
                    hit = hit and rejected_resize(R.resize_fwd(c["x"], c["out"], plant=plant)[0], ref, u, T)
                hits[plant] += hit
    print("resize mutants rejected on (cases x dtypes):", hits)
    assert all(v > 0 for v in hits.values()), hits


def rejected_resize(got, ref, unit, T):
    return R.excess(got, ref, unit, K_RESIZE, T == BF16) > K_RESIZE


def test_resize_adjoint_window_covers_every_tap():
    """The gather-form adjoint visits the outputs [lo, hi] that R.resize_window computes in the kernels' float32 arithmetic:
    every output whose float32 taps touch source index i must lie inside, for every extent pair of the cases. Without the
    clamp of hi at the last source index the window is the same on all of them: the generic bound already reaches
    n_out - 1 there (src(n_out - 1) < n_in), so that line is a safeguard no test can tell from its absence."""
    pairs = {(a[k], b[k]) for a, b in PC.RESIZE_CASES.values() for k in (0, 1)}
    for n_in, n_out in sorted(pairs):
        i0, i1, l1 = R.resize_taps(n_out, n_in, F32)
        for i in range(n_in):
            touching = [o for o in range(n_out) if (int(i0[o]) == i and l1[o] < 1) or (int(i1[o]) == i and l1[o] > 0)]
            lo, hi = R.resize_window(i, n_in, n_out)
            assert not touching or (lo <= touching[0] and touching[-1] <= hi), (n_in, n_out, i)
            assert R.resize_window(i, n_in, n_out, last_row_clamp=False) == (lo, hi), (n_in, n_out, i)
