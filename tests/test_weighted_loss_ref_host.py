"""CPU: tests/weighted_loss_ref.py (the float64 statement of the weighted / smoothed cross entropy, the focal loss, their
fusion with soft Dice and the label histogram) against torch.nn.functional and torch.autograd in float64, so that
tests/test_weighted_loss_kernels_gpu.py, which holds the kernels to it, does not depend on the kernels; what it does with stray
labels and with batches that have no valid pixel or no weight; and that the bound of the GPU file (4 x max(float32 yardstick,
floor), see there) is tight enough to catch seven planted errors on that file's small cases.

Planted errors (test_planted_errors_exceed_the_bound prints the figures; "old gates" are those of the module-level file
tests/test_weighted_loss_gpu.py, loss |d| <= 2e-6 and gradient max-rel <= 1e-4 against the batch's largest gradient):
    error planted                                   error / bound, smallest .. largest over 12 cases   old gates
    S replaced by K in the smoothing gradient         1.5e4 .. 4.7e4                                     caught
    smoothing term normalised by n_valid, not W       2.9e4 .. 7.7e4                                     caught
    w[y] dropped from the normaliser                  4.3e5 .. 1.4e6                                     caught
    alpha[y] read as alpha[k]                         1.8e5 .. 5.2e5                                     caught
    the focal lead term dropped                       7.2e4 .. 2.0e5                                     caught
    class 0's Dice I and T sums swapped               2.4e5 .. 6.3e5                                     caught
    one gradient element left at zero                 1.0e3 .. 6.8e5                                     caught
Evaluated on these inputs the old gates would have caught every one of them as well (0 of 12 cases let through): what the suite
lacked was not a tighter gate but a launch that reaches the code in question with a reference beside it (the second grid trip,
K beyond 5, the unaligned fallback), and a bound that does not lean on the batch's largest gradient."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import tail_ref as tr
from tests import weighted_loss_ref as wr
from tests.helpers import max_rel
from tests.test_weighted_loss_kernels_gpu import CE_GRID, FOCAL_GRID, FUSED_MODES, IGN, MIXES, SMALL_SHAPES, block_case, class_weights

LOSS_FLOOR, GRAD_FLOOR = 1e-6, 2e-8
OLD_LOSS_GATE, OLD_GRAD_GATE = 2e-6, 1e-4


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _targets(shape, K, seed, ignore_frac=0.2):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, K, shape, generator=g)
    t = torch.where(torch.rand(shape, generator=g) < ignore_frac, torch.full_like(t, IGN), t)
    t.view(-1)[0] = 0
    return t


def _close(a, b, rel=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300)


def focal_written_out(logits, target, gamma, alpha):
    """mean over valid pixels of alpha[y] (1 - p_y)^gamma (-log p_y), for autograd."""
    logp = torch.log_softmax(logits, dim=1)
    valid = target != IGN
    safe = torch.where(valid, target, torch.zeros_like(target))
    lp = logp.gather(1, safe.unsqueeze(1)).squeeze(1)
    a = torch.ones_like(lp) if alpha is None else alpha.to(logits.dtype)[safe]
    per = a * (1.0 - lp.exp()).pow(gamma) * (-lp)
    return (per * valid).sum() / valid.sum()


# ---- in-range labels against torch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("eps,zero", CE_GRID)
def test_cross_entropy_w_against_torch(K, eps, zero):
    lg, tg = _rnd((3, K, 61), 10 + K, 3.0), _targets((3, 61), K, 20 + K)
    w = class_weights(K, zero).double()
    a = lg.clone().requires_grad_(True)
    ref = F.cross_entropy(a, tg, weight=w, ignore_index=IGN, label_smoothing=eps)
    ref.backward()
    loss, d = wr.cross_entropy_w(lg, tg, w, eps, IGN)
    assert _close(loss, ref.detach()) and _close(d, a.grad)
    if eps == 0.0:
        loss1, d1 = wr.cross_entropy_w(lg, tg, torch.ones(K), 0.0, IGN)
        base, dbase = tr.cross_entropy(lg, tg, IGN)
        assert _close(loss1, base) and _close(d1, dbase)
        lossn, dn = wr.cross_entropy_w(lg, tg, None, 0.0, IGN)
        assert torch.equal(lossn, loss1) and torch.equal(dn, d1)


@pytest.mark.parametrize("K", [2, 3, 5, 16])
@pytest.mark.parametrize("gamma,alpha", FOCAL_GRID)
def test_focal_against_autograd(K, gamma, alpha):
    lg, tg = _rnd((3, K, 61), 30 + K, 1.5), _targets((3, 61), K, 40 + K)
    a_vec = class_weights(K).double() if alpha else None
    a = lg.clone().requires_grad_(True)
    ref = focal_written_out(a, tg, gamma, a_vec)
    ref.backward()
    loss, d = wr.focal(lg, tg, gamma, a_vec, IGN)
    assert _close(loss, ref.detach(), 1e-11) and _close(d, a.grad, 1e-11)
    if gamma == 0.0 and not alpha:
        base, dbase = tr.cross_entropy(lg, tg, IGN)
        assert _close(loss, base) and _close(d, dbase)


def test_focal_with_one_class_is_zero():
    lg, tg = _rnd((2, 1, 9), 3, 3.0), _targets((2, 9), 1, 4)
    loss, d = wr.focal(lg, tg, 2.0, torch.tensor([0.7]), IGN)
    assert float(loss) == 0.0 and torch.equal(d, torch.zeros_like(d))
    loss, d = wr.focal(lg, tg, 0.0, None, IGN)
    assert float(loss) == 0.0 and torch.equal(d, torch.zeros_like(d))


def test_focal_stays_accurate_in_float32_on_confident_pixels():
    """What the cancellation-free form is for: with q down to 1e-30 the float32 evaluation of the target class's gradient is
    within 1e-4 of its float64 value per element, where a 1 - p_t form returns 0."""
    K = 2
    lg, tg = (_rnd((2, K, 512), 5, 24.0)).float(), _targets((2, 512), K, 6)
    (r, rd), (f, fd) = wr.focal(lg.double(), tg, 2.0, None, IGN), wr.focal(lg, tg, 2.0, None, IGN)
    sel = rd.abs() > 1e-30
    assert int(((rd.abs() < 1e-12) & sel).sum()) > 100
    assert float(((fd.double() - rd).abs() / rd.abs().clamp_min(1e-300))[sel].max()) <= 1e-4
    assert abs(float(f) - float(r)) <= 1e-5 * float(r)


@pytest.mark.parametrize("K", [1, 2, 4, 6])
@pytest.mark.parametrize("mode", list(FUSED_MODES))
def test_dice_ce_w_is_the_weighted_sum_of_its_parts(K, mode):
    kind, eps, gamma = FUSED_MODES[mode]
    w = None if kind is None else class_weights(K, kind == "zero").double()
    lg, tg = _rnd((2, K, 45), 50 + K, 3.0), _targets((2, 45), K, 60 + K)
    di, ddi = tr.soft_dice(lg, tg, IGN, 0.7)
    if gamma is None:
        term, dterm = wr.cross_entropy_w(lg, tg, w, eps, IGN)
    else:
        term, dterm = wr.focal(lg, tg, gamma, w, IGN)
    for wce, wd in MIXES:
        comb, t, d, grad = wr.dice_ce_w(lg, tg, w, eps, gamma, 0.7, wce, wd, IGN)
        assert torch.equal(t, term) and torch.equal(d, di)
        assert _close(comb, wce * term + wd * di) and _close(grad, wce * dterm + wd * ddi)
    I, P, T = wr.dice_sums(lg, tg, IGN)
    num, den = 2.0 * I + 0.7, P + T + 0.7
    assert _close(1.0 - (num / den).sum() / K, di) and int(T.sum()) == int((tg != IGN).sum())


def test_label_hist_is_bincount():
    tg = _targets((3, 500), 5, 70)
    h = wr.label_hist(tg, 5, IGN)
    flat = tg.reshape(-1)
    assert h.dtype == torch.int64 and torch.equal(h[:5], torch.bincount(flat[flat != IGN], minlength=5))
    assert int(h[5]) == int((flat == IGN).sum()) and int(h.sum()) == flat.numel()


# ---- stray labels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_stray_labels_are_ignored_pixels(dtype):
    K = 3
    lg, tg = _rnd((2, K, 200), 80, 3.0).to(dtype), _targets((2, 200), K, 81)
    stray = torch.tensor([-1, K, 254, -2 ** 63])
    at = torch.arange(4, 200, 9)
    tg[1, at] = stray[torch.arange(len(at)) % 4]
    clean = tg.clone()
    clean[1, at] = IGN
    assert not bool(wr.valid(tg, K, IGN)[1, at].any()) and torch.equal(wr.valid(tg, K, IGN), clean != IGN)
    w = class_weights(K)
    for fn in (lambda t: wr.cross_entropy_w(lg, t, w, 0.1, IGN), lambda t: wr.focal(lg, t, 2.0, w, IGN),
               lambda t: wr.dice_ce_w(lg, t, w, 0.1, None, 1.0, 0.3, 0.7, IGN), lambda t: wr.dice_ce_w(lg, t, None, 0.0, 0.5, 1.0, 0.3, 0.7, IGN),
               lambda t: wr.soft_dice(lg, t, IGN), lambda t: wr.dice_sums(lg, t, IGN)):
        for a, b in zip(fn(tg), fn(clean)):
            assert torch.equal(a, b)
    h, hc = wr.label_hist(tg, K, IGN), wr.label_hist(clean, K, IGN)
    assert torch.equal(h[:K], hc[:K]) and int(hc[K]) - int(h[K]) == len(at) and int(h.sum()) == tg.numel() - len(at)
    # the logits under a pixel that is not valid are never looked at
    dirty = lg.clone()
    dirty[:, :, :][(~wr.valid(tg, K, IGN)).unsqueeze(1).expand_as(lg)] = float("nan")
    for a, b in zip(wr.dice_ce_w(dirty, tg, w, 0.1, None, 1.0, 0.3, 0.7, IGN), wr.dice_ce_w(lg, tg, w, 0.1, None, 1.0, 0.3, 0.7, IGN)):
        assert torch.equal(a, b)
    for a, b in zip(wr.focal(dirty, tg, 2.0, w, IGN), wr.focal(lg, tg, 2.0, w, IGN)):
        assert torch.equal(a, b)


# ---- degenerate batches ----------------------------------------------------------------------------------------------------
def test_all_ignored_batch_is_pinned():
    """No valid pixel (ignored or stray): CE_w and focal are 0/0 = NaN, Dice is 0, the combined loss NaN, every gradient
    element exactly 0, in float64 and in float32. The GPU test asserts exactly this."""
    K = 3
    lg = _rnd((2, K, 16), 90, 3.0)
    tg = torch.full((2, 16), IGN)
    tg[1] = K
    w = class_weights(K)
    for dt in (torch.float64, torch.float32):
        x = lg.to(dt)
        for loss, d in (wr.cross_entropy_w(x, tg, w, 0.1, IGN), wr.focal(x, tg, 2.0, w, IGN), wr.focal(x, tg, 0.0, None, IGN)):
            assert math.isnan(float(loss)) and torch.equal(d, torch.zeros_like(d))
        for eps, gamma in ((0.1, None), (0.0, 2.0)):
            comb, term, di, d = wr.dice_ce_w(x, tg, w, eps, gamma, 1.0, 0.3, 0.7, IGN)
            assert math.isnan(float(comb)) and math.isnan(float(term)) and float(di) == 0.0 and torch.equal(d, torch.zeros_like(d))
        assert float(wr.normaliser(tg, K, w, IGN, dt)) == 0.0
    assert wr.label_hist(tg, K, IGN).tolist() == [0, 0, 0, 16]


def test_only_zero_weight_classes_valid_is_pinned():
    """Every valid pixel in a class of weight 0: W = 0, the weighted CE is 0/0 = NaN (torch gives the same), the gradient of an
    invalid pixel stays exactly 0; focal with alpha = 0 there is a plain 0 (its normaliser is n_valid)."""
    K = 3
    lg = _rnd((2, K, 40), 91, 3.0)
    tg = torch.where(_targets((2, 40), K, 92) == IGN, IGN, 1)
    w = class_weights(K).double()
    w[1] = 0.0
    loss, d = wr.cross_entropy_w(lg, tg, w, 0.0, IGN)
    assert math.isnan(float(loss)) and bool((d[(tg == IGN).unsqueeze(1).expand_as(d)] == 0).all())
    assert math.isnan(float(F.cross_entropy(lg, tg, weight=w, ignore_index=IGN)))
    comb, term, di, d = wr.dice_ce_w(lg, tg, w, 0.0, None, 1.0, 0.3, 0.7, IGN)
    assert math.isnan(float(comb)) and math.isnan(float(term)) and math.isfinite(float(di))
    assert torch.equal(di, tr.soft_dice(lg, tg, IGN)[0])
    loss, d = wr.focal(lg, tg, 2.0, w, IGN)
    assert float(loss) == 0.0 and torch.equal(d, torch.zeros_like(d))


# ---- planted errors --------------------------------------------------------------------------------------------------------
def _softmax_parts(lg, tg):
    K = lg.shape[1]
    v = wr.valid(tg, K, IGN)
    safe = torch.where(v, tg, torch.zeros_like(tg))
    own = torch.zeros(lg.shape, dtype=torch.bool).scatter_(1, safe.unsqueeze(1), True)
    return v, safe, own, torch.softmax(lg, 1)


def _mut_S_is_K(lg, tg, w, eps):
    """S replaced by K in the smoothing gradient."""
    K = lg.shape[1]
    v, _, _, p = _softmax_parts(lg, tg)
    loss, d = wr.cross_entropy_w(lg, tg, w, eps, IGN)
    W = wr.normaliser(tg, K, w, IGN)
    return loss, d + torch.where(v.unsqueeze(1), (eps / K) * (K - w.sum()) * p / W, torch.zeros_like(p))


def _mut_smoothing_by_n(lg, tg, w, eps):
    """The smoothing term normalised by n_valid instead of W."""
    K = lg.shape[1]
    loss, d = wr.cross_entropy_w(lg, tg, w, eps, IGN)
    hard, dhard = wr.cross_entropy_w(lg, tg, w, 0.0, IGN)
    ratio = wr.normaliser(tg, K, w, IGN) / wr.normaliser(tg, K, None, IGN)
    return (1 - eps) * hard + (loss - (1 - eps) * hard) * ratio, (1 - eps) * dhard + (d - (1 - eps) * dhard) * ratio


def _mut_normaliser_without_w(lg, tg, w, eps):
    """w[y] dropped from the normaliser."""
    K = lg.shape[1]
    loss, d = wr.cross_entropy_w(lg, tg, w, eps, IGN)
    ratio = wr.normaliser(tg, K, w, IGN) / wr.normaliser(tg, K, None, IGN)
    return loss * ratio, d * ratio


def _mut_alpha_k(lg, tg, alpha, gamma):
    """alpha[y] read as alpha[k] in the gradient."""
    _, safe, _, _ = _softmax_parts(lg, tg)
    loss, d = wr.focal(lg, tg, gamma, alpha, IGN)
    return loss, d / alpha[safe].unsqueeze(1) * alpha.reshape(1, -1, 1)


def _mut_no_lead(lg, tg, alpha, gamma):
    """The focal lead term g q^(g-1) p_t log p_t dropped."""
    v, safe, own, p = _softmax_parts(lg, tg)
    loss, _ = wr.focal(lg, tg, gamma, alpha, IGN)
    q = 1.0 - (p * own).sum(1)
    c = (alpha[safe] * (-q.pow(gamma)) / v.sum()).unsqueeze(1)
    return loss, torch.where(v.unsqueeze(1), c * torch.where(own, q.unsqueeze(1), -p), torch.zeros_like(p))


def _mut_dice_swap(lg, tg, w, eps, wce, wd):
    """Class 0's Dice sums I and T swapped (in the loss and in the derivative that is built from them)."""
    K = lg.shape[1]
    v, _, own, p = _softmax_parts(lg, tg)
    oh = (own & v.unsqueeze(1)).double()
    I, P, T = wr.dice_sums(lg, tg, IGN)
    I, T = I.clone(), T.clone()
    I[0], T[0] = T[0].clone(), I[0].clone()
    num, den = (2.0 * I + 1.0).reshape(1, K, 1), (P + T + 1.0).reshape(1, K, 1)
    dice = 1.0 - (num / den).sum() / K
    g = -(2.0 * oh * den - num) / (den * den) / K
    ddice = torch.where(v.unsqueeze(1), p * (g - (p * g).sum(1, keepdim=True)), torch.zeros_like(p))
    term, dterm = wr.cross_entropy_w(lg, tg, w, eps, IGN)
    return (wce * term + wd * dice, term, dice), wce * dterm + wd * ddice


def _mut_one_zero(lg, tg, w, eps):
    """One gradient element never written (the last pixel of a grid-stride trip): modelled as a zero, in the lightest class
    (weight 0.2) of the last valid pixel."""
    loss, d = wr.cross_entropy_w(lg, tg, w, eps, IGN)
    d = d.clone()
    last = int(wr.valid(tg[-1], lg.shape[1], IGN).nonzero().max())
    assert float(d[-1, 0, last]) != 0.0
    d[-1, 0, last] = 0.0
    return loss, d


def _figures(mut_loss, mut_grad, r, f, scale, grad_floor=GRAD_FLOOR):
    """(largest error / bound over the loss and the gradient, would the module-level gates have passed it)."""
    (r_loss, rd), (f_loss, fd) = r, f
    lerr, lbound = abs(float(mut_loss) - float(r_loss)), 4.0 * max(abs(float(f_loss) - float(r_loss)), LOSS_FLOOR)
    gerr = float((mut_grad - rd).abs().max()) * scale
    gbound = 4.0 * max(float((fd.double() - rd).abs().max()) * scale, grad_floor)
    old = lerr <= OLD_LOSS_GATE and max_rel(mut_grad, rd) <= OLD_GRAD_GATE
    return max(lerr / lbound, gerr / gbound), old


def _planted(name, lg, tg, K):
    l64, l32 = lg.double(), lg.float()
    w = class_weights(K)
    wd64 = w.double()
    W, n = float(wr.normaliser(tg, K, w, IGN)), float(wr.normaliser(tg, K, None, IGN))
    if name in ("S is K", "smoothing by n", "normaliser without w", "one element zero"):
        fn = {"S is K": _mut_S_is_K, "smoothing by n": _mut_smoothing_by_n, "normaliser without w": _mut_normaliser_without_w,
              "one element zero": _mut_one_zero}[name]
        ml, md = fn(l64, tg, wd64, 0.1)
        return _figures(ml, md, wr.cross_entropy_w(l64, tg, w, 0.1, IGN), wr.cross_entropy_w(l32, tg, w, 0.1, IGN), W / float(w.max()))
    if name in ("alpha[k]", "no lead"):
        fn = _mut_alpha_k if name == "alpha[k]" else _mut_no_lead
        ml, md = fn(l64, tg, wd64, 2.0)
        return _figures(ml, md, wr.focal(l64, tg, 2.0, w, IGN), wr.focal(l32, tg, 2.0, w, IGN), n / float(w.max()))
    assert name == "dice I, T swapped"
    (mc, mt, mdi), md = _mut_dice_swap(l64, tg, wd64, 0.1, 0.3, 0.7)
    r, f = wr.dice_ce_w(l64, tg, w, 0.1, None, 1.0, 0.3, 0.7, IGN), wr.dice_ce_w(l32, tg, w, 0.1, None, 1.0, 0.3, 0.7, IGN)
    a = _figures(mc, md, (r[0], r[3]), (f[0], f[3]), W / float(w.max()))
    b = _figures(mdi, md, (r[2], r[3]), (f[2], f[3]), W / float(w.max()))
    return max(a[0], b[0]), a[1] and b[1]


PLANTED = ["S is K", "smoothing by n", "normaliser without w", "alpha[k]", "no lead", "dice I, T swapped", "one element zero"]
ONE_BLOCK = [(1, 255), (1, 256), (1, 257)]


@pytest.mark.parametrize("name", PLANTED)
def test_planted_errors_exceed_the_bound(name):
    """Each mutated float64 formula, on the GPU file's cases around one block at K = 2 .. 5, against the bound that file
    computes from the float32 yardstick: beyond it on at least one case (in fact on every one)."""
    ratios, old = [], []
    for K in (2, 3, 4, 5):
        for B, HW in ONE_BLOCK:
            lg, tg = block_case(B, K, HW)
            ratio, passed_old = _planted(name, lg, tg, K)
            ratios.append(ratio)
            old.append(passed_old)
    print("PLANTED %-22s | error / bound: smallest %.3g, largest %.3g over %d cases | the old module-level gates pass it on %d of %d cases"
          % (name, min(ratios), max(ratios), len(ratios), sum(old), len(old)))
    assert max(ratios) > 1.0, (name, ratios)


def test_unmutated_reference_is_inside_the_bound():
    """The same machinery on the formulas as they are gives 0: the planted-error figures measure the mutation alone."""
    lg, tg = block_case(1, 3, 257)
    w = class_weights(3)
    r, f = wr.cross_entropy_w(lg.double(), tg, w, 0.1, IGN), wr.cross_entropy_w(lg.float(), tg, w, 0.1, IGN)
    assert _figures(r[0], r[1], r, f, 1.0) == (0.0, True)


# ---- which of floor and yardstick sets each bound --------------------------------------------------------------------------
def test_print_yardstick_over_floor():
    """Largest float32 yardstick / floor per output over the GPU file's small cases: below 1 the floor sets the bound, above 1
    the yardstick does. Printed, and required to be finite and below 1e3 (a yardstick that large would make the bound vacuous)."""
    worst = {}

    def note(key, yard, floor):
        worst[key] = max(worst.get(key, 0.0), yard / floor)

    for K in (2, 3, 4, 5):
        for B, HW in SMALL_SHAPES:
            lg, tg = block_case(B, K, HW)
            l64, l32 = lg.double(), lg.float()
            n = float(wr.normaliser(tg, K, None, IGN))
            for eps, zero in CE_GRID:
                w = class_weights(K, zero)
                (r, rd), (f, fd) = wr.cross_entropy_w(l64, tg, w, eps, IGN), wr.cross_entropy_w(l32, tg, w, eps, IGN)
                scale = float(wr.normaliser(tg, K, w, IGN)) / float(w.max())
                note("ce_w loss", abs(float(f) - float(r)), LOSS_FLOOR)
                note("ce_w gradient * W / max w", float((fd.double() - rd).abs().max()) * scale, GRAD_FLOOR)
            for gamma, alpha in FOCAL_GRID:
                a = class_weights(K) if alpha else None
                (r, rd), (f, fd) = wr.focal(l64, tg, gamma, a, IGN), wr.focal(l32, tg, gamma, a, IGN)
                note("focal loss", abs(float(f) - float(r)), LOSS_FLOOR)
                note("focal gradient * n / max alpha", float((fd.double() - rd).abs().max()) * n / (float(a.max()) if alpha else 1.0), GRAD_FLOOR)
            for mode, (kind, eps, gamma) in FUSED_MODES.items():
                w = None if kind is None else class_weights(K, kind == "zero")
                for wce, wd in MIXES:
                    r, f = (wr.dice_ce_w(x, tg, w, eps, gamma, 1.0, wce, wd, IGN) for x in (l64, l32))
                    norm = n if gamma is not None else float(wr.normaliser(tg, K, w, IGN))
                    scale = 1.0 if wce == 0.0 else norm / (1.0 if w is None else float(w.max()))
                    for i, what in enumerate(("combined", "term", "dice")):
                        note("dice_ce_w %s" % what, abs(float(f[i]) - float(r[i])), LOSS_FLOOR)
                    note("dice_ce_w gradient (Dice alone)" if wce == 0.0 else "dice_ce_w gradient * norm / max w",
                         float((f[3].double() - r[3]).abs().max()) * scale, GRAD_FLOOR)
    for key, ratio in worst.items():
        print("YARDSTICK %-36s | largest float32 yardstick / floor %8.3f | the bound is set by the %s"
              % (key, ratio, "yardstick" if ratio > 1.0 else "floor"))
        assert math.isfinite(ratio) and ratio < 1e3, (key, ratio)
