"""Host: tests/bn_chain_ref.py (the float64 reference the BatchNorm-backward kernels are judged by) against torch.autograd.

The unit is built in float64 torch on the CPU — F.batch_norm -> ReLU -> SELayer gate (two bias-free Linears, sigmoid;
Unet-ChannalAttention.py:45-72, 82-86), optionally with a MaxPool2d(2) branch or a 1x1 output conv behind it — and
differentiated by autograd; the reference's finalize -> se_forward -> reduce -> coef -> apply chain must give the same
numbers to 1e-12 max-rel. Nothing here touches a kernel: this is what makes the reference independent of them."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_chain_ref as R

F64 = torch.float64
TOL = 1e-12


def _max_rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("form", ["plain", "pool", "outc"])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("use_se", [1, 0])
def test_reference_chain_is_autograd(use_se, training, relu, form):
    g = torch.Generator().manual_seed(17 + 8 * use_se + 4 * training + 2 * relu + len(form))
    B, H, W, C, Cr, K = 3, 4, 6, 8, 2, 3
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    y = (rnd(B, H, W, C) * (0.5 + torch.rand(C, generator=g, dtype=F64)) + 3 * rnd(C)).requires_grad_()
    gamma, beta, cbias = (rnd(C) + 1.5).requires_grad_(), (0.3 * rnd(C)).requires_grad_(), rnd(C).requires_grad_()
    w1, w2 = (0.5 * rnd(Cr, C)).requires_grad_(), (0.5 * rnd(C, Cr)).requires_grad_()
    rm0, rv0 = rnd(C), torch.rand(C, generator=g, dtype=F64) + 0.5
    wout, bout = rnd(K, C).requires_grad_(), rnd(K).requires_grad_()
    momentum, eps = 0.1, 1e-5

    # ---- torch
    rm, rv = rm0.clone(), rv0.clone()
    x = _nchw(y) + cbias[None, :, None, None]
    a = F.batch_norm(x, rm, rv, gamma, beta, bool(training), momentum, eps)
    z = torch.relu(a) if relu else a
    if use_se:
        sq_t = z.mean((2, 3))
        hid_t = torch.relu(sq_t @ w1.T)
        gate_t = torch.sigmoid(hid_t @ w2.T)
        out = z * gate_t[:, :, None, None]
    else:
        out = z
    dskip, dpooled, dl = rnd(B, H, W, C), rnd(B, H // 2, W // 2, C), rnd(B, K, H, W)
    if form == "plain":
        loss = (out * _nchw(dskip)).sum()
    elif form == "pool":
        loss = (out * _nchw(dskip)).sum() + (F.max_pool2d(out, 2) * _nchw(dpooled)).sum()
    else:
        loss = (F.conv2d(out, wout[:, :, None, None], bout) * dl).sum()
    params = [y, gamma, beta, cbias] + ([w1, w2] if use_se else []) + ([wout, bout] if form == "outc" else [])
    grads = dict(zip(["dy", "dgamma", "dbeta", "dcb", "dW1", "dW2"][:4 + 2 * use_se] + ["dwout", "dbout"],
                     torch.autograd.grad(loss, params)))

    # ---- the reference chain
    yd = y.detach()
    part = torch.stack([yd.sum(2), (yd * yd).sum(2)], 2).reshape(B * H, 2, C)         # one partial row per image row
    fin, _ = R.finalize(part, B * H * W, gamma.detach(), beta.detach(), cbias.detach(), rm0, rv0, 5, momentum, eps, training)
    assert _max_rel(fin["running_mean"], rm) <= TOL and _max_rel(fin["running_var"], rv) <= TOL
    assert fin["num_batches_tracked"] == 5 + training
    sc, sh, mu, istd = fin["scale"], fin["shift"], fin["mean"], fin["invstd"]
    assert _max_rel(_nchw(yd * sc + sh), a.detach()) <= TOL
    se = {}
    if use_se:
        fwd, _ = R.se_forward(yd, sc, sh, w1.detach(), w2.detach(), relu)
        assert _max_rel(fwd["sq"], sq_t.detach()) <= TOL and _max_rel(fwd["hid"], hid_t.detach()) <= TOL
        assert _max_rel(fwd["gate"], gate_t.detach()) <= TOL
        se = dict(pooled=fwd["pooled"], sq=fwd["sq"], hid=fwd["hid"], gate=fwd["gate"], w1=w1.detach(), w2=w2.detach())
    if form == "plain":
        dout = dskip
    elif form == "pool":
        arg = R.pool_arg(_nhwc(out.detach()))
        idx = F.max_pool2d(out.detach(), 2, return_indices=True)[1]                    # flat h*W + w of the maximum
        assert torch.equal(arg.to(torch.int64), _nhwc((idx // W) % 2 * 2 + (idx % W) % 2))
        dout = R.pool_dout(dskip, dpooled, arg, F64)
    else:
        dout, _ = R.outc_dout(dl, wout.detach(), F64)
        wp, _ = R.outc_wpart(dl, wout.shape, yd, sc, sh, se.get("gate"), relu, 3, F64)
        fold = wp.sum(0)
        assert _max_rel(fold[:K * C].reshape(K, C), grads["dwout"]) <= TOL and _max_rel(fold[K * C:], grads["dbout"]) <= TOL
    for rpp in (1, 3, H):
        red, _ = R.reduce(dout, yd, sc, sh, relu, rpp)
        c, _ = R.coef(red, H, W, sc, sh, mu, istd, training, use_se, **se)
        for form_k in ("k", "part"):
            if form_k == "part" and not training:
                continue
            kk = dict(k1=c["k1"], k2=c["k2"]) if form_k == "k" else dict(tb=c["tb"], tg=c["tg"])
            dy, _ = R.apply(dout, yd, sc, sh, mu, istd, relu, se.get("gate"), c.get("coefB"), **kk)
            assert _max_rel(dy, grads["dy"]) <= TOL
        assert _max_rel(c["dgamma"], grads["dgamma"]) <= TOL and _max_rel(c["dbeta"], grads["dbeta"]) <= TOL
        if training:
            assert float(c["dconv_bias"].abs().max()) == 0 and float(grads["dcb"].abs().max()) <= TOL * float(grads["dbeta"].abs().max())
            xhat = (yd - mu) * istd
            scale_dy = float(dy.abs().sum((0, 1, 2)).max())
            assert float(dy.sum((0, 1, 2)).abs().max()) <= TOL * scale_dy                  # sum dy = 0 per channel
            # sum dy*xhat = scale * dgamma * (1 - sum xhat^2 / N), and sum xhat^2 / N = var / (var + eps): zero but for eps
            resid = (dy * xhat).sum((0, 1, 2)) - sc * c["dgamma"] * eps * istd * istd
            assert float(resid.abs().max()) <= TOL * scale_dy * float(xhat.abs().max())
        else:
            assert _max_rel(c["dconv_bias"], grads["dcb"]) <= TOL
        if use_se:
            assert _max_rel(c["dW1"], grads["dW1"]) <= TOL and _max_rel(c["dW2"], grads["dW2"]) <= TOL


def test_float32_evaluation_is_a_floor_not_the_reference():
    """dt=float32 runs the same formulas in naive float32: close to, and not equal to, the float64 values, and within the
    rule's unit (the procedure that fixes k; tests/test_bn_backward_chain_gpu.py records the figures)."""
    g = torch.Generator().manual_seed(3)
    B, H, W, C = 2, 5, 7, 8
    y = (torch.randn(B, H, W, C, generator=g) + 30.0).float()
    dout = torch.randn(B, H, W, C, generator=g).float()
    sc, sh = torch.full((C,), 0.7), torch.full((C,), -21.0)
    ref, unit = R.reduce(dout, y, sc, sh, 1, 2)
    lo, _ = R.reduce(dout, y, sc, sh, 1, 2, dt=torch.float32)
    r = R.ratio(lo, ref, unit)
    assert 0 < r < 1.0
