"""CPU: tests/tail_ref.py (the float64 statement of the output head, the losses, the confusion counts and Adam) against
torch.nn.functional, torch.autograd, oracle.soft_dice_loss and torch.optim.Adam in float64, so that the GPU tests that hold
the kernels to it do not depend on the kernels; the exact-representability of every integer case those tests run; and what
the reference does for a batch without a valid pixel."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ca_oracle as orc
from tests import tail_ref as tr

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _targets(shape, K, seed, ignore_frac=0.2):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, K, shape, generator=g)
    return torch.where(torch.rand(shape, generator=g) < ignore_frac, torch.full_like(t, 255), t)


# ---- output head -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
def test_head_against_conv2d_autograd(bias):
    x, w, b, dl = _rnd((2, 12, 3, 5), 1), _rnd((3, 12), 2), _rnd((3,), 3), _rnd((2, 3, 3, 5), 4)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.conv2d(xr, wr[:, :, None, None], br if bias else None)
    ref.backward(dl)
    assert torch.allclose(tr.head_forward(x, w, b if bias else None), ref.detach(), rtol=0, atol=1e-12)
    dx, dW, db = tr.head_backward(x, w, dl)
    assert torch.allclose(dx, xr.grad, rtol=0, atol=1e-12) and torch.allclose(dW, wr.grad, rtol=0, atol=1e-12)
    assert torch.allclose(db, dl.sum((0, 2, 3)), rtol=0, atol=1e-12)
    if bias:
        assert torch.allclose(db, br.grad, rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gate", [True, False])
def test_head_input_from_y_is_the_rounded_gated_relu(dtype, gate):
    y = _rnd((2, 8, 3, 4), 5, 3.0).to(dtype).double()
    gen = torch.Generator().manual_seed(17)
    scale, shift = torch.rand(8, generator=gen) + 0.5, (_rnd((8,), 6) * 0.5).float()
    g = torch.rand(2, 8, generator=gen) + 0.25 if gate else None
    z = tr.head_input_from_y(y, scale, shift, g, dtype)
    exact = torch.relu(y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    if gate:
        exact = exact * g.double().view(2, 8, 1, 1)
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23
    assert float((z - exact).abs().max()) <= ulp * float(exact.abs().max())
    assert torch.equal(z, z.to(dtype).double()) and float(z.min()) >= 0.0
    # the ReLU decision is that of the float32 fused multiply-add
    fma = (y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).float()
    assert bool((z[fma <= 0] == 0).all()) and bool((z[fma > 0] > 0).all())


def test_every_integer_head_case_is_exactly_representable():
    """|logit| and |dW|, |db| partial sums below 2^24 (bounded by the sums of absolute terms, so in any order), |dx| <= 256,
    operands within the stated ranges, and the case list covers what the GPU file promises."""
    cases = tr.head_case_list()
    assert len({c[0] for c in cases}) == len(cases)
    for seed, (cid, dt, C, K, (B, H, W), bias) in enumerate(cases):
        c = tr.head_case(seed, B, C, H, W, K, bias)
        tr.assert_head_case_exact(c)
        assert float(c.x.abs().max()) <= 8 and float(c.w.abs().max()) <= 4 and float(c.dl.abs().max()) <= 4
        for t in (c.x, c.w, c.dl, c.logits, c.dx, c.dW, c.db):
            assert torch.equal(t, t.round())
        assert torch.equal(c.x, c.x.to(DT[dt]).double()) and torch.equal(c.dx, c.dx.to(DT[dt]).double())
        assert torch.equal(c.logits, c.logits.float().double()) and torch.equal(c.dW, c.dW.float().double())
        assert (c.bias is None) == (not bias)
    have = {(dt, C, K) for _, dt, C, K, _, _ in cases}
    assert all((dt, C, K) in have for dt, C in tr.NARROW + tr.WIDE for K in tr.KS)
    assert {("bf16", 512, 7), ("bf16", 512, 8)} <= have
    assert all((dt, C, geo) in {(d, c, g) for _, d, c, _, g, _ in cases} for dt, C in tr.NARROW + tr.WIDE for geo in tr.GEOMETRIES)
    assert any(not b for *_, b in cases)
    assert [tr.is_wide(dt, C) for dt, C in tr.NARROW + tr.WIDE] == [False] * 6 + [True] * 4


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("gate", [True, False])
def test_integer_fromy_case_is_exactly_representable(dt, gate):
    c = tr.fromy_case(3, 2, 64, 3, 5, 3, gate, DT[dt])
    tr.assert_fromy_case_exact(c, DT[dt])
    exact = torch.relu(c.y * c.scale.view(1, -1, 1, 1) + c.shift.view(1, -1, 1, 1))
    exact = exact * c.gate.view(2, 64, 1, 1) if gate else exact
    assert torch.equal(c.z, exact)                               # no rounding anywhere: z is the real-number value
    assert float((c.z == 0).double().mean()) > 0.1 and float((c.z > 0).double().mean()) > 0.1


# ---- losses ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K", [((2, 7, 9), 2), ((3, 5, 4), 5), ((1, 1, 1), 3), ((2, 6, 6), 1)])
def test_losses_against_autograd(shape, K):
    lg = _rnd((shape[0], K) + shape[1:], 7, 3.0)
    tg = _targets(shape, K, 8)
    tg.view(-1)[0] = 0                                           # at least one valid pixel
    a = lg.clone().requires_grad_(True)
    ce = F.cross_entropy(a, tg, ignore_index=255)
    ce.backward()
    loss, d = tr.cross_entropy(lg, tg, 255)
    assert abs(float(loss) - float(ce.detach())) <= 1e-13 and torch.allclose(d, a.grad, rtol=0, atol=1e-14)
    b = lg.clone().requires_grad_(True)
    di = orc.soft_dice_loss(b, tg, 255, smooth=0.7)
    di.backward()
    loss, d = tr.soft_dice(lg, tg, 255, 0.7)
    assert abs(float(loss) - float(di.detach())) <= 1e-13 and torch.allclose(d, b.grad, rtol=0, atol=1e-14)
    c = lg.clone().requires_grad_(True)
    both = 0.3 * orc.cross_entropy(c, tg) + 0.7 * orc.soft_dice_loss(c, tg, 255, smooth=1.0)
    both.backward()
    loss, lce, ldi, d = tr.dice_ce(lg, tg, 255, 1.0, 0.3, 0.7)
    assert abs(float(loss) - float(both.detach())) <= 1e-13 and torch.allclose(d, c.grad, rtol=0, atol=1e-14)
    assert abs(float(lce) - float(ce.detach())) <= 1e-13


def test_losses_with_saturated_logits_are_finite_and_exact():
    """A spread of 160 between the classes, with and without 3e4 on top: p is exactly 0 / 1 in float64 and float32, the loss
    is 160 x the share of wrong pixels, the gradient of the saturated class 0 or -1/n."""
    K, shape = 3, (2, 8, 8)
    tg = _targets(shape, K, 9, 0.1)
    hot = torch.randint(0, K, shape, generator=torch.Generator().manual_seed(10))
    for base in (0.0, 3e4):
        lg = torch.full((2, K, 8, 8), base, dtype=torch.float64)
        lg.scatter_(1, hot.unsqueeze(1), base + 160.0)
        for dt in (torch.float64, torch.float32):
            loss, d = tr.cross_entropy(lg.to(dt), tg)
            valid = tg != 255
            n = int(valid.sum())
            wrong = int((valid & (hot != tg)).sum())
            assert bool(torch.isfinite(d).all()) and abs(float(loss) - 160.0 * wrong / n) <= 1e-4
            sat = d.gather(1, hot.unsqueeze(1)).squeeze(1)
            want = torch.where(valid & (hot != tg), 1.0 / n, 0.0).to(dt)
            assert float((sat - want).abs().max()) <= 1e-7 / n
            ld, dd = tr.soft_dice(lg.to(dt), tg)
            assert math.isfinite(float(ld)) and bool(torch.isfinite(dd).all())


def test_all_ignored_batch_is_pinned():
    """No valid pixel: CE is 0/0 = NaN (as torch's), Dice is 0 (every class term is smooth / smooth), the combined loss NaN,
    and every gradient element is exactly 0 — in float64 and in float32. The GPU test asserts exactly this."""
    lg = _rnd((2, 3, 4, 4), 11, 3.0)
    tg = torch.full((2, 4, 4), 255)
    for dt in (torch.float64, torch.float32):
        loss, d = tr.cross_entropy(lg.to(dt), tg)
        assert math.isnan(float(loss)) and torch.equal(d, torch.zeros_like(d))
        loss, d = tr.soft_dice(lg.to(dt), tg)
        assert float(loss) == 0.0 and torch.equal(d, torch.zeros_like(d))
        loss, ce, di, d = tr.dice_ce(lg.to(dt), tg)
        assert math.isnan(float(loss)) and math.isnan(float(ce.detach())) and float(di) == 0.0 and torch.equal(d, torch.zeros_like(d))
    a = lg.clone().requires_grad_(True)
    ref = F.cross_entropy(a, tg, ignore_index=255)
    ref.backward()
    assert math.isnan(float(ref.detach())) and torch.equal(a.grad, torch.zeros_like(a.grad))
    assert torch.equal(tr.confusion(lg, tg, 3), torch.zeros(3, 3, dtype=torch.int64))
    # one image wholly ignored is nothing special: its gradient rows are 0, the other image carries the loss
    tg2 = tg.clone()
    tg2[1] = _targets((4, 4), 3, 12, 0.0)
    loss, d = tr.cross_entropy(lg, tg2)
    assert math.isfinite(float(loss)) and torch.equal(d[0], torch.zeros_like(d[0])) and float(d[1].abs().max()) > 0


def test_confusion_counts_ties_and_oracle():
    lg = _rnd((3, 4, 5, 7), 13)
    tg = _targets((3, 5, 7), 4, 14)
    tp, fp, fn = orc.confusion_counts(lg, tg, 4)
    got = tr.confusion(lg, tg, 4)
    assert got.tolist() == [list(map(int, tp)), list(map(int, fp)), list(map(int, fn))]
    tie = torch.zeros(1, 3, 1, 4, dtype=torch.float64)
    tie[0, :, 0, 1] = torch.tensor([1.0, 2.0, 2.0])              # classes 1 and 2 tie: 1 wins
    tie[0, :, 0, 2] = torch.tensor([-1.0, -1.0, -1.0])           # all three tie: 0 wins
    tie[0, :, 0, 3] = torch.tensor([0.0, 0.0, 5.0])
    t = torch.tensor([[[0, 2, 1, 255]]])
    assert tr.confusion(tie, t, 3).tolist() == [[1, 0, 0], [1, 1, 0], [0, 1, 1]]


# ---- Adam ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", [1.0, 0.25])
def test_adam_reference_against_torch_optim(gscale):
    p0 = _rnd((257,), 15)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    rp, rm, rv = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 5):
        g = _rnd((257,), 20 + step)
        p.grad = g * gscale
        opt.step()
        rp, rm, rv = tr.adam_reference(rp, g, rm, rv, step, 1e-3, 0.9, 0.999, 1e-8, gscale)
        assert float((rp - p.detach()).abs().max()) <= 1e-14
    st = opt.state[p]
    assert torch.allclose(rm, st["exp_avg"], rtol=1e-13, atol=0) and torch.allclose(rv, st["exp_avg_sq"], rtol=1e-13, atol=0)
    # g = 0 on v = 0: nothing moves
    q, m, v = tr.adam_reference(p0, torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros_like(p0), 1)
    assert torch.equal(q, p0) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0
