"""Reference statement of the imbalance-aware losses (csrc/loss_weighted.hip: insar_cross_entropy_w, insar_focal,
insar_dice_ce_w, insar_label_hist), written in plain torch from the formulas in that file's header and DESIGN.md
"Imbalance-aware losses", with every gradient in closed form (no autograd) and without the package.
tests/test_weighted_loss_ref_host.py holds it to torch.nn.functional and torch.autograd in float64;
tests/test_weighted_loss_kernels_gpu.py holds the kernels to it.

Every function computes in the dtype of `logits`: float64 is the reference, the same call on float32 tensors is the "plain
float32" evaluation whose deviation from float64 is the GPU tests' yardstick (the rule of tests/test_loss_kernels_gpu.py).

logits [B][K][HW], target [B][HW] int64, w [K] class weights (alpha for focal), p = softmax over k.
    v_i = [y_i != ignore and 0 <= y_i < K]      (a stray label counts as ignored), n = sum v, W = sum_i v_i w[y_i], S = sum_c w_c
    CE_w  = [(1-e) sum_i v_i w[y_i] nll_{i,y_i} + (e/K) sum_i v_i sum_c w_c nll_{i,c}] / W,     nll_{i,c} = -log p_{i,c}
            dCE_w/dz_{i,k} = v_i [(1-e) w[y_i] (p_{i,k} - d_{k,y_i}) + (e/K) (S p_{i,k} - w_k)] / W
    focal = sum_i v_i a[y_i] q^g (-log p_t) / n,   p_t = p_{i,y_i},  q = 1 - p_t
            dfocal/dz_{i,k} = v_i a[y_i] [g q^(g-1) p_t log p_t - q^g] (d_{k,y_i} - p_{i,k}) / n
Focal is written without cancellation, so that its float32 evaluation stays a meaningful yardstick on confident pixels: q from
the log-sum-exp of the OTHER classes, -log p_t = log1p(e^x) with x = lse(others) - z_t (as max(x, 0) + log1p(e^-|x|), which
float32 evaluates for x > 88 too), the target class's d_{t,t} - p_t is q itself; q^g = 1 for g = 0 and 0 for q = 0, g q^(g-1) p_t log p_t = 0 for g = 0 and for q = 0.
A pixel that is not valid gets gradient 0 by selection and none of its logits (NaN and inf included) reaches a sum: with no
valid pixel the CE forms are 0/0 = NaN and every gradient element is exactly 0."""
import torch

from tests import tail_ref as tr


def valid(target, K, ignore=255):
    return (target != ignore) & (target >= 0) & (target < K)


def _parts(logits, target, ignore):
    """(logits with the invalid pixels' values replaced by 0, valid [B][HW], safe target, one-hot [B][K][HW] bool)."""
    K = logits.shape[1]
    v = valid(target, K, ignore)
    lg = torch.where(v.unsqueeze(1), logits, torch.zeros_like(logits))
    safe = torch.where(v, target, torch.zeros_like(target))
    own = torch.zeros(lg.shape, dtype=torch.bool).scatter_(1, safe.unsqueeze(1), True)
    return lg, v, safe, own


def _vec(w, K, dtype):
    return torch.ones(K, dtype=dtype) if w is None else w.to(dtype)


def normaliser(target, K, weight=None, ignore=255, dtype=torch.float64):
    """W (the count of valid pixels when weight is None)."""
    v = valid(target, K, ignore)
    safe = torch.where(v, target, torch.zeros_like(target))
    return torch.where(v, _vec(weight, K, dtype)[safe], torch.zeros((), dtype=dtype)).sum()


def cross_entropy_w(logits, target, weight, eps=0.0, ignore=255):
    """(loss, dlogits) in logits.dtype."""
    lg, v, safe, own = _parts(logits, target, ignore)
    K, dt = lg.shape[1], lg.dtype
    w = _vec(weight, K, dt)
    zero = torch.zeros((), dtype=dt)
    mx = lg.max(1, keepdim=True).values
    e = torch.exp(lg - mx)
    se = e.sum(1, keepdim=True)
    nll = (mx + torch.log(se)) - lg                                        # [B][K][HW]
    p = e / se
    wy = torch.where(v, w[safe], zero)                                     # [B][HW]
    W, S = wy.sum(), w.sum()
    wk = w.reshape(1, K, 1)
    hard = (wy * torch.where(own, nll, zero).sum(1)).sum()
    soft = torch.where(v, (wk * nll).sum(1), zero).sum()
    loss = ((1.0 - eps) * hard + (eps / K) * soft) / W
    d = ((1.0 - eps) * wy.unsqueeze(1) * (p - own.to(dt)) + (eps / K) * (S * p - wk)) / W
    return loss, torch.where(v.unsqueeze(1), d, zero)


def focal(logits, target, gamma, alpha=None, ignore=255):
    """(loss, dlogits) in logits.dtype; alpha None: ones."""
    lg, v, safe, own = _parts(logits, target, ignore)
    K, dt = lg.shape[1], lg.dtype
    a = _vec(alpha, K, dt)
    zero, one = torch.zeros((), dtype=dt), torch.ones((), dtype=dt)
    lse = torch.logsumexp(lg, dim=1)
    others = torch.logsumexp(lg.masked_fill(own, float("-inf")), dim=1)    # -inf for K = 1: q = 0
    zt = lg.gather(1, safe.unsqueeze(1)).squeeze(1)
    logq = others - lse
    q = torch.exp(logq)
    x = others - zt                                                        # -log p_t = log1p(e^x), without overflow for x > 88
    nll = torch.clamp_min(x, 0.0) + torch.log1p(torch.exp(-x.abs()))
    pt = torch.exp(zt - lse)
    p = torch.exp(lg - lse.unsqueeze(1))
    if gamma == 0:
        qg, lead = torch.ones_like(q), torch.zeros_like(q)
    else:
        pos = q > 0
        fin = torch.where(pos, logq, zero)
        qg = torch.where(pos, torch.exp(gamma * fin), zero)
        lead = torch.where(pos, gamma * torch.exp((gamma - 1.0) * fin) * pt * (-nll), zero)
    n = v.sum().to(dt)
    ay = torch.where(v, a[safe], zero)
    loss = (ay * qg * nll).sum() / n
    c = (ay * (lead - qg) / n).unsqueeze(1)
    d = c * torch.where(own, q.unsqueeze(1), -p)
    return loss, torch.where(v.unsqueeze(1), d, zero)


def _dice_inputs(logits, target, ignore):
    lg, v, _, _ = _parts(logits, target, ignore)
    return lg, torch.where(v, target, torch.full_like(target, ignore))


def soft_dice(logits, target, ignore=255, smooth=1.0):
    """tail_ref.soft_dice over the validity rule above: (loss, dlogits)."""
    lg, t = _dice_inputs(logits, target, ignore)
    return tr.soft_dice(lg, t, ignore, smooth)


def dice_sums(logits, target, ignore=255):
    """(I [K], P [K], T [K]) of the Dice term, in logits.dtype."""
    lg, v, _, own = _parts(logits, target, ignore)
    oh = (own & v.unsqueeze(1)).to(lg.dtype)
    p = torch.softmax(lg, dim=1) * v.unsqueeze(1).to(lg.dtype)
    return (p * oh).sum((0, 2)), p.sum((0, 2)), oh.sum((0, 2))


def dice_ce_w(logits, target, weight=None, eps=0.0, gamma=None, smooth=1.0, ce_weight=1.0, dice_weight=1.0, ignore=255):
    """(combined, term, dice, dlogits): ce_weight * term + dice_weight * Dice; term is focal(gamma, alpha = weight) when gamma
    is not None and cross_entropy_w(weight or ones, eps) otherwise."""
    if gamma is None:
        term, dterm = cross_entropy_w(logits, target, weight, eps, ignore)
    else:
        term, dterm = focal(logits, target, gamma, weight, ignore)
    di, ddi = soft_dice(logits, target, ignore, smooth)
    return ce_weight * term + dice_weight * di, term, di, ce_weight * dterm + dice_weight * ddi


def label_hist(target, K, ignore=255):
    """int64 [K+1]: pixels per class, then pixels equal to ignore; any other label is counted nowhere."""
    t = target.reshape(-1)
    out = torch.zeros(K + 1, dtype=torch.int64)
    for c in range(K):
        out[c] = int((t == c).sum()) if c != ignore else 0
    out[K] = int((t == ignore).sum())
    return out
