"""Host: tests/attention_ref.py (the float64 reference the attention kernels are judged by) against torch.autograd.

SpatialAttention (Unet-SpatialAttention.py:59-82) and the ChannelAttentionModule (DeepLabV3-ChannelAttention.py:49-79) are
composed in float64 from torch primitives and differentiated by autograd; the reference's per-launch functions, chained
in launch order, must give the same output, input gradient and parameter gradients to 1e-10 max-rel. Nothing here touches
a kernel: this is what makes the reference independent of them. The last tests run the float32 evaluation that fixes the
GPU file's tolerance, and show that a deliberately wrong reference (a tap off by one, the last instead of the first
arg-max) lies far outside it."""
import pytest
import torch
import torch.nn.functional as F

from tests import attention_ref as A
from tests import bn_chain_ref as R

F64 = torch.float64
TOL = 1e-10


def _max_rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _separated(g, B, H, W, C):
    """Noise whose per-pixel channel maximum (and per-channel spatial maximum) stands clear of the runner-up."""
    x = torch.randn(B, H, W, C, generator=g, dtype=F64)
    x.view(-1, C)[torch.arange(B * H * W), torch.randint(0, C, (B * H * W,), generator=g)] += 4.0
    return x


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("shape,rows", [((2, 3, 4, 8), 3), ((1, 5, 2, 16), 7), ((3, 1, 6, 8), 1)])
def test_sa_reference_chain_is_autograd(shape, rows, training):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(12 + 2 * C + training + H)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x = _separated(g, B, H, W, C).requires_grad_()
    w1, b1, w2, b2 = (0.5 * rnd(1, 2, 3, 3)).requires_grad_(), rnd(1).requires_grad_(), rnd(1, 1, 3, 3).requires_grad_(), rnd(1).requires_grad_()
    ga1, be1, ga2, be2 = (rnd(1) + 1.5).requires_grad_(), (0.3 * rnd(1)).requires_grad_(), (rnd(1) - 1.5).requires_grad_(), (0.5 + 0.3 * rnd(1)).requires_grad_()
    rm1, rv1, rm2, rv2 = 0.2 * rnd(1), torch.rand(1, generator=g, dtype=F64) + 0.5, 0.2 * rnd(1), torch.rand(1, generator=g, dtype=F64) + 0.5
    dout = rnd(B, H, W, C)
    momentum, eps = 0.1, 1e-5

    # ---- torch
    xn = _nchw(x)
    a = torch.cat([xn.mean(1, keepdim=True), xn.max(1, keepdim=True).values], 1)
    r1, q1, r2, q2 = rm1.clone(), rv1.clone(), rm2.clone(), rv2.clone()
    h1 = torch.relu(F.batch_norm(F.conv2d(a, w1, b1, padding=1), r1, q1, ga1, be1, bool(training), momentum, eps))
    zz = torch.relu(F.batch_norm(F.conv2d(h1, w2, b2, padding=1), r2, q2, ga2, be2, bool(training), momentum, eps))
    out = xn * torch.sigmoid(zz)
    params = [x, w1, b1, ga1, be1, w2, b2, ga2, be2]
    gr = dict(zip(["dx", "dw1", "db1", "dgamma1", "dbeta1", "dw2", "db2", "dgamma2", "dbeta2"],
                  torch.autograd.grad((out * _nchw(dout)).sum(), params)))

    # ---- the reference, launch by launch
    xd, M = x.detach(), B * H * W
    cp, _ = A.sa_compress(xd)
    assert torch.equal(cp["arg"], xd.argmax(3))
    comp = torch.stack([cp["mean"], cp["max"]], -1)
    c1, _ = A.sa_conv(1, comp, w1.detach(), None, rows, training)
    f1, _ = R.finalize(c1["stat"], M, ga1.detach(), be1.detach(), b1.detach(), rm1, rv1, 0, momentum, eps, training)
    bn1 = [f1[k].reshape(()) for k in ("scale", "shift", "mean", "invstd")]
    c2, _ = A.sa_conv(2, c1["z"], w2.detach(), torch.stack(bn1 + bn1), rows, training)
    f2, _ = R.finalize(c2["stat"], M, ga2.detach(), be2.detach(), b2.detach(), rm2, rv2, 0, momentum, eps, training)
    bn = torch.stack(bn1 + [f2[k].reshape(()) for k in ("scale", "shift", "mean", "invstd")])
    if training:
        assert _max_rel(f1["running_mean"], r1) <= TOL and _max_rel(f2["running_var"], q2) <= TOL
    else:
        assert c1["stat"] is None and c2["stat"] is None
    gt, _ = A.sa_gate(xd, c2["z"], bn)
    assert _max_rel(_nchw(gt["out"]), out.detach()) <= TOL
    assert not training or 0 < float((gt["s"] > 0.5).double().mean()) < 1      # normalised: both sides of the outer ReLU are met
    ds, _ = A.sa_dscale(xd, dout, c2["z"], gt["s"], bn, rows)
    part = torch.full((rows, A.SA_PART_COLS), 0.0, dtype=F64)
    part[:, :2] = ds["part"]
    k2, _ = A.sa_bwd_coef(2, part, M, training)
    s2, _ = A.sa_bwd_stencil(2, ds["g2"], c2["z"], bn, k2["coef"], w2.detach(), c1["z"], rows)
    part[:, :12] = s2["part"]
    k1, _ = A.sa_bwd_coef(1, part, M, training)
    s1, _ = A.sa_bwd_stencil(1, s2["g1"], c1["z"], bn, k1["coef"], w1.detach(), comp, rows)
    part[:, :19] = s1["part"]
    k0, _ = A.sa_bwd_coef(0, part, M, training)
    dx, _ = A.sa_dx(dout, gt["s"], s1["dcomp"], cp["arg"])
    assert _max_rel(dx, gr["dx"]) <= TOL
    got = dict(dw1=k0["dw1"].reshape(1, 2, 3, 3), dw2=k1["dw2"].reshape(1, 1, 3, 3), dgamma1=k1["dgamma1"], dbeta1=k1["dbeta1"],
               dgamma2=k2["dgamma2"], dbeta2=k2["dbeta2"])
    for k, v in got.items():
        assert _max_rel(v.reshape(gr[k].shape), gr[k]) <= TOL, k
    for k, v, scale in (("db1", k0["db1"], bn[0].abs() * s2["g1"].abs().sum()), ("db2", k1["db2"], bn[4].abs() * ds["g2"].abs().sum())):
        if training:      # a bias in front of a training-mode BatchNorm has no gradient: zero up to rounding
            assert abs(float(v)) <= TOL * float(scale) and abs(float(gr[k])) <= TOL * float(scale)
        else:
            assert _max_rel(v.reshape(gr[k].shape), gr[k]) <= TOL, k
            assert float(k1["coef"].abs().max()) == 0 and float(k2["coef"].abs().max()) == 0


@pytest.mark.parametrize("shape,Cr,rpp", [((2, 4, 5, 8), 2, 1), ((3, 7, 3, 16), 4, 3), ((1, 2, 2, 4), 1, 5)])
def test_cam_reference_chain_is_autograd(shape, Cr, rpp):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(5 + C + rpp)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x = _separated(g, B, H, W, C)
    x.view(B, H * W, C)[:, torch.randint(0, H * W, (1,), generator=g)] += 1.0
    x = (x + 0.3).requires_grad_()
    w1, w2 = rnd(Cr, C).requires_grad_(), rnd(C, Cr).requires_grad_()
    dout = rnd(B, H, W, C)

    xn = _nchw(x)
    mlp = lambda t: F.conv2d(torch.relu(F.conv2d(t, w1[:, :, None, None])), w2[:, :, None, None])
    gate_t = torch.sigmoid(mlp(F.adaptive_avg_pool2d(xn, 1)) + mlp(F.adaptive_max_pool2d(xn, 1)))
    out = xn * gate_t
    gdx, gw1, gw2 = torch.autograd.grad((out * _nchw(dout)).sum(), [x, w1, w2])

    xd = x.detach()
    pl, _ = A.cam_pool(xd, rpp)
    ex, _ = A.cam_excite(pl["psum"], pl["pmax"], pl["parg"], w1.detach(), w2.detach(), H, W)
    assert torch.equal(ex["arg"], xd.reshape(B, H * W, C).argmax(1)) and torch.equal(ex["mx"], xd.amax((1, 2)))
    assert _max_rel(ex["gate"], gate_t.detach().reshape(B, C)) <= TOL
    assert B * Cr == 1 or bool((ex["pre_a"] > 0).any() or (ex["pre_m"] > 0).any()) and bool((ex["pre_a"] < 0).any() or (ex["pre_m"] < 0).any())
    one, zero = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)
    red, _ = R.reduce(dout, xd, one, zero, 0, rpp)
    bw, _ = A.cam_bwd_coef(red, ex["gate"], ex["ha"], ex["hm"], ex["avg"], ex["mx"], w1.detach(), w2.detach(), H, W)
    dx = dout * ex["gate"][:, None, None, :] + bw["coefB"][:, None, None, :]
    dx, _ = A.cam_scatter_max(dx, bw["dmax"], ex["arg"], F64)
    assert _max_rel(dx, gdx) <= TOL and _max_rel(bw["dW1"], gw1) <= TOL and _max_rel(bw["dW2"], gw2) <= TOL


# ------------------------------------------------------------------------------------------------ the float32 floor
def _sa_inputs(seed=4, B=2, H=5, W=6, C=16):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(x=rn(B, H, W, C), comp=rn(B, H, W, 2), dz=rn(B, H, W), z=rn(B, H, W), w1=rn(1, 2, 3, 3), w2=rn(1, 1, 3, 3),
                bn=torch.tensor([1.0, 0.1, 0.0, 1.0, -0.8, 0.2, 0.1, 0.9]), k=torch.tensor([0.01, -0.02, 0.03, 0.01]))


def test_float32_evaluation_is_a_floor_not_the_reference():
    """dt=float32 runs the same formulas in naive float32: close to, and not equal to, the float64 values, within the unit."""
    c = _sa_inputs()
    for fn in (lambda dt: A.sa_conv(1, c["comp"], c["w1"], c["bn"], 3, 1, dt),
               lambda dt: A.sa_bwd_stencil(1, c["dz"], c["z"], c["bn"], c["k"][2:], c["w1"], c["comp"], 3, dt),
               lambda dt: A.sa_bwd_stencil(2, c["dz"], c["z"], c["bn"], c["k"][:2], c["w2"], c["z"] + 0.3, 3, dt)):
        (ref, unit), (lo, _) = fn(F64), fn(torch.float32)
        for k in ref:
            assert 0 < R.ratio(lo[k], ref[k], unit[k]) < 2.0, k


def test_a_wrong_reference_lies_far_outside_the_floor():
    """What the GPU tests would see from a kernel that is right, judged by a reference that is subtly wrong: the float32
    evaluation of the right formulas against a float64 evaluation with one tap moved by a pixel, a work-group's rows taken
    at the wrong stride, and the last instead of the first arg-max."""
    c = _sa_inputs()
    lo, _ = A.sa_conv(1, c["comp"], c["w1"], c["bn"], 3, 1, torch.float32)
    ref, unit = A.sa_conv(1, c["comp"], c["w1"], c["bn"], 3, 1)
    wrong_w = c["w1"].clone()
    wrong_w[0, 0, 0] = wrong_w[0, 0, 0].roll(1)                                   # the top row of taps, one pixel to the right
    bad, _ = A.sa_conv(1, c["comp"], wrong_w, c["bn"], 3, 1)
    assert R.ratio(lo["z"], ref["z"], unit["z"]) < 2 and R.ratio(lo["z"], bad["z"], unit["z"]) > 1e4
    bad, _ = A.sa_conv(1, c["comp"], c["w1"], c["bn"], 4, 1)                        # rows b, b + 4, ... instead of b, b + 3, ...
    assert R.ratio(lo["stat"], ref["stat"], unit["stat"]) < 2 and R.ratio(lo["stat"][:3], bad["stat"][:3], unit["stat"]) > 1e4
    lo, _ = A.sa_bwd_stencil(1, c["dz"], c["z"], c["bn"], c["k"][2:], c["w1"], c["comp"], 3, torch.float32)
    ref, unit = A.sa_bwd_stencil(1, c["dz"], c["z"], c["bn"], c["k"][2:], c["w1"], c["comp"], 3)
    bad, _ = A.sa_bwd_stencil(1, c["dz"], c["z"], c["bn"], c["k"][2:], c["w1"].flip(3), c["comp"], 3)   # conv instead of conv^T in x
    assert R.ratio(lo["dcomp"], ref["dcomp"], unit["dcomp"]) < 2 and R.ratio(lo["dcomp"], bad["dcomp"], unit["dcomp"]) > 1e4
    # ties: the first occurrence wins, in both families
    x = torch.zeros(1, 2, 3, 8)
    x[0, 0, 0, 1] = x[0, 0, 0, 5] = 1.0
    x[0, 0, 2, 3] = x[0, 1, 0, 3] = 2.0
    assert int(A.sa_compress(x)[0]["arg"][0, 0, 0]) == 1
    for rpp in (1, 2):
        pl, _ = A.cam_pool(x, rpp)
        ex, _ = A.cam_excite(pl["psum"], pl["pmax"], pl["parg"], torch.ones(1, 8), torch.ones(8, 1), 2, 3)
        assert int(ex["arg"][0, 3]) == 2 and float(ex["mx"][0, 3]) == 2.0
    x[0, 1, 1, 3] = float("nan")
    pl, _ = A.cam_pool(x, 1)
    ex, _ = A.cam_excite(pl["psum"], pl["pmax"], pl["parg"], torch.ones(1, 8), torch.ones(8, 1), 2, 3)
    assert int(ex["arg"][0, 3]) == 4 and bool(torch.isnan(ex["mx"][0, 3])) and not bool(torch.isnan(ex["mx"][0, 2]))
    # scatter: one element per (image, channel), rounded once from the float32 sum
    dx = torch.ones(1, 2, 3, 8, dtype=torch.bfloat16)
    got, _ = A.cam_scatter_max(dx, torch.full((1, 8), 2.0 ** -9), torch.full((1, 8), 5), torch.bfloat16)
    assert int((got != dx).sum()) == 0                                             # 1 + 2^-9 rounds to even: back to 1
    got, _ = A.cam_scatter_max(dx, torch.full((1, 8), 3 * 2.0 ** -9), torch.full((1, 8), 5), torch.bfloat16)
    assert bool((got[0, 1, 2] == 1 + 2.0 ** -7).all()) and int((got != dx).sum()) == 8
