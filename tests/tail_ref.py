"""Reference statement of the tail of a training step — the 1x1 output head (csrc/direct.hip: conv1x1_out_*), the losses, the
confusion counts and Adam (csrc/loss_optim.hip) — written from the formulas in the kernels' comments and include/insar_hip.h
in plain torch / numpy, not through autograd. tests/test_tail_ref_host.py holds it to torch.nn.functional, torch.autograd,
oracle.soft_dice_loss and torch.optim.Adam in float64; the three GPU files (test_output_head_gpu.py, test_loss_kernels_gpu.py,
test_adam_kernel_gpu.py) hold the kernels to it.

Every function computes in the dtype of its floating operands: float64 is the reference, the same call on float32 tensors
is the "plain float32" evaluation whose deviation from float64 the loss tests use as their yardstick.

Output head.  x [B][C][H][W], w [K][C], bias [K] or None:
    logits[n,k,h,w] = bias[k] + sum_c w[k,c] x[n,c,h,w]
    dx[n,c,h,w] = sum_k dl[n,k,h,w] w[k,c];   dW[k,c] = sum_{n,h,w} dl[n,k,h,w] x[n,c,h,w];   db[k] = sum_{n,h,w} dl[n,k,h,w]
Integer operands (x in [-8, 8], w, bias, dl in [-4, 4]) make every one of these an integer that fp32 holds exactly under any
summation order and that bf16 holds exactly where it is stored (dx): a kernel then has ONE right answer (head_case).

Losses.  logits [B][K][...], target [B][...] int64, v = 1[target != ignore_index], n = sum v, p = softmax over k:
    CE   = (1/n) sum_pixels v (logsumexp - logit[target]);      dCE/dlogit_k = v (p_k - 1[target = k]) / n
    Dice = 1 - mean_k (2 I_k + s) / (P_k + T_k + s),  I_k = sum v p_k 1[t=k],  P_k = sum v p_k,  T_k = sum v 1[t=k]
           dDice/dp_k = g_k = -(1/K) (2 1[t=k] den_k - num_k) / den_k^2;   dDice/dlogit_k = v p_k (g_k - sum_j p_j g_j)
An ignored pixel's gradient is 0 by selection, not by multiplication: with n = 0 the CE is 0/0 = NaN and every gradient
element is exactly 0 (test_tail_ref_host.py pins that, and that torch does the same)."""
from types import SimpleNamespace

import numpy as np
import torch

SUM_LIMIT = 2 ** 24      # integers below 2^24 in magnitude: every fp32 partial sum of them, in any partition, is exact
OUT_LIMIT = 256          # |v| <= 256: an integer that bf16 (8 significant bits) holds exactly


# ---- output head ---------------------------------------------------------------------------------------------------------
def head_forward(x_nchw, w, bias=None):
    out = torch.einsum("bchw,kc->bkhw", x_nchw, w)
    return out if bias is None else out + bias.reshape(1, -1, 1, 1)


def head_backward(x_nchw, w, dl):
    """(dx [B][C][H][W], dW [K][C], db [K])."""
    return torch.einsum("bkhw,kc->bchw", dl, w), torch.einsum("bkhw,bchw->kc", dl, x_nchw), dl.sum((0, 2, 3))


def head_input_from_y(y, scale, shift, gate, dtype):
    """z = round_T(relu(y*scale + shift) * gate[n]): what conv1x1_out_bwd_kernel<T, FROMY> recomputes as the head's input.
    y [B][C][H][W] holds values of T; scale, shift [C] and gate [B][C] (or None) hold float32 values. y*scale + shift is one
    fused multiply-add in float32: the float64 value (the product of two 24-bit significands is exact there) rounded to
    float32 once. ReLU, the float32 multiply by the gate, then the rounding to T. Returned in float64."""
    t = (y.double() * scale.double().reshape(1, -1, 1, 1) + shift.double().reshape(1, -1, 1, 1)).float()
    t = torch.clamp_min(t, 0.0)
    if gate is not None:
        t = t * gate.float().reshape(gate.shape[0], -1, 1, 1)
    return t.to(dtype).double()


def head_case(seed, B, C, H, W, K, bias=True):
    """Seeded integer operands of one head launch with its exact results, all float64 holding integers:
    x in [-8, 8], w, bias, dl in [-4, 4]; logits, dx, dW, db from the functions above."""
    gen = torch.Generator().manual_seed(seed)

    def ints(shape, a):
        return torch.randint(-a, a + 1, shape, generator=gen, dtype=torch.int64).double()

    x, w, b, dl = ints((B, C, H, W), 8), ints((K, C), 4), ints((K,), 4), ints((B, K, H, W), 4)
    b = b if bias else None
    dx, dW, db = head_backward(x, w, dl)
    return SimpleNamespace(x=x, w=w, bias=b, dl=dl, logits=head_forward(x, w, b), dx=dx, dW=dW, db=db, B=B, C=C, H=H, W=W, K=K)


def head_case_bounds(c):
    """What makes the case's answer unique: (largest |sum of |terms|| of a logit, of a dW / db element, largest |dx|). Any
    partial sum of a logit or of a folded partial is bounded by the sum of the absolute terms."""
    lg = torch.einsum("bchw,kc->bkhw", c.x.abs(), c.w.abs()) + (0 if c.bias is None else c.bias.abs().reshape(1, -1, 1, 1))
    dw = torch.einsum("bkhw,bchw->kc", c.dl.abs(), c.x.abs())
    dxa = torch.einsum("bkhw,kc->bchw", c.dl.abs(), c.w.abs())
    return float(lg.max()), max(float(dw.max()), float(c.dl.abs().sum((0, 2, 3)).max())), float(dxa.max())


def assert_head_case_exact(c):
    lg, dw, dx = head_case_bounds(c)
    assert lg < SUM_LIMIT and dw < SUM_LIMIT and dx <= OUT_LIMIT, (lg, dw, dx)


def fromy_case(seed, B, C, H, W, K, gate, dtype):
    """Integer y in [-8, 8], scale in {1/2, 1, 2}, shift in {-2, ..., 2}, gate in {1/2, 1, 2} (or None): z is then a multiple
    of 1/4 of magnitude <= 36, exact in fp32 and bf16, and every dl*z product a multiple of 1/4 below 2^24 / 4."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.randint(-8, 9, (B, C, H, W), generator=gen).double()
    pw = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    scale = pw[torch.randint(0, 3, (C,), generator=gen)]
    shift = torch.randint(-2, 3, (C,), generator=gen).double()
    g = pw[torch.randint(0, 3, (B, C), generator=gen)] if gate else None
    w = torch.randint(-4, 5, (K, C), generator=gen).double()
    dl = torch.randint(-4, 5, (B, K, H, W), generator=gen).double()
    z = head_input_from_y(y, scale, shift, g, dtype)
    _, dW, db = head_backward(z, w, dl)
    return SimpleNamespace(y=y, scale=scale, shift=shift, gate=g, w=w, dl=dl, z=z, dW=dW, db=db, B=B, C=C, H=H, W=W, K=K)


def assert_fromy_case_exact(c, dtype):
    z4 = c.z * 4.0
    assert torch.equal(z4, z4.round()) and float(c.z.abs().max()) <= 36.0
    assert torch.equal(c.z, c.z.to(dtype).double())
    assert 4.0 * float(torch.einsum("bkhw,bchw->kc", c.dl.abs(), c.z.abs()).max()) < SUM_LIMIT


# ---- losses --------------------------------------------------------------------------------------------------------------
def _flat(logits, target):
    B, K = logits.shape[0], logits.shape[1]
    return logits.reshape(B, K, -1), target.reshape(B, -1)


def _onehot(t, valid, K, dtype):
    safe = torch.where(valid, t, torch.zeros_like(t))
    oh = torch.zeros((t.shape[0], K, t.shape[1]), dtype=dtype)
    oh.scatter_(1, safe.unsqueeze(1), 1.0)
    return oh * valid.unsqueeze(1).to(dtype)


def _softmax(lg):
    e = torch.exp(lg - lg.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def cross_entropy(logits, target, ignore_index=255):
    """(loss, dlogits) in logits.dtype."""
    lg, t = _flat(logits, target)
    valid = t != ignore_index
    oh = _onehot(t, valid, lg.shape[1], lg.dtype)
    mx = lg.max(1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(lg - mx).sum(1, keepdim=True))).squeeze(1)
    n = valid.sum().to(lg.dtype)
    per_pixel = torch.where(valid, lse - (lg * oh).sum(1), torch.zeros_like(lse))
    loss = per_pixel.sum() / n
    d = torch.where(valid.unsqueeze(1), (_softmax(lg) - oh) / n, torch.zeros_like(lg))
    return loss, d.reshape(logits.shape)


def soft_dice(logits, target, ignore_index=255, smooth=1.0):
    """(loss, dlogits) in logits.dtype."""
    lg, t = _flat(logits, target)
    K = lg.shape[1]
    valid = t != ignore_index
    v = valid.unsqueeze(1).to(lg.dtype)
    oh = _onehot(t, valid, K, lg.dtype)
    p = _softmax(lg)
    inter, psum, tsum = (p * oh).sum((0, 2)), (p * v).sum((0, 2)), oh.sum((0, 2))
    num, den = 2.0 * inter + smooth, psum + tsum + smooth
    loss = 1.0 - (num / den).sum() / K
    g = -(2.0 * oh * den.reshape(1, K, 1) - num.reshape(1, K, 1)) / (den * den).reshape(1, K, 1) / K
    d = p * (g - (p * g).sum(1, keepdim=True))
    d = torch.where(valid.unsqueeze(1), d, torch.zeros_like(d))
    return loss, d.reshape(logits.shape)


def dice_ce(logits, target, ignore_index=255, smooth=1.0, ce_weight=1.0, dice_weight=1.0):
    """(combined loss, CE, Dice, dlogits): ce_weight * CE + dice_weight * Dice."""
    ce, dce = cross_entropy(logits, target, ignore_index)
    di, ddi = soft_dice(logits, target, ignore_index, smooth)
    return ce_weight * ce + dice_weight * di, ce, di, ce_weight * dce + dice_weight * ddi


def confusion(logits, target, K, ignore=255):
    """int64 [3][K]: TP, FP, FN over the pixels with target != ignore; the prediction is the arg-max with ties going to the
    LOWER class index."""
    lg, t = _flat(logits, target)
    pred = np.argmax(lg.numpy(), axis=1)                       # numpy: the first maximum
    t = t.numpy()
    valid = t != ignore
    out = np.zeros((3, K), dtype=np.int64)
    for c in range(K):
        out[0, c] = np.count_nonzero(valid & (pred == c) & (t == c))
        out[1, c] = np.count_nonzero(valid & (pred == c) & (t != c))
        out[2, c] = np.count_nonzero(valid & (pred != c) & (t == c))
    return torch.from_numpy(out)


# ---- Adam ----------------------------------------------------------------------------------------------------------------
def adam_reference(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0):
    """One step, float64, new (p, m, v):  g' = gscale g;  m = m + (g' - m)(1 - b1);  v = b2 v + (1 - b2) g'^2;
    p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),  bc1 = 1 - b1^step,  bc2 = 1 - b2^step."""
    p, g, m, v = p.double(), g.double() * gscale, m.double(), v.double()
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps))
    return p, m, v


# ---- the integer cases of tests/test_output_head_gpu.py (listed here so that the host test can check every one) -----------
NARROW = [("f32", 16), ("f32", 64), ("f32", 256), ("bf16", 64), ("bf16", 256), ("bf16", 512)]
WIDE = [("f32", 512), ("f32", 260), ("bf16", 1024), ("bf16", 520)]       # 260 / 520: cpp = 65, only lane 0 owns a second chunk
KS = [1, 2, 3, 8]
# (B, H, W): one-pixel rows; a row that is no whole number of waves; more than one pass of 256 threads at cpp = 16; more rows
# than insar_conv1x1_out_bwd_blocks returns (1050 > 1024); a single row
GEOMETRIES = [(2, 3, 1), (2, 3, 5), (1, 2, 37), (2, 525, 3), (1, 1, 7)]


def head_case_list():
    """[(id, dtype name, C, K, (B, H, W), bias)]: every width at every geometry (K rotating through KS), every width at
    every K (at 2 x 3 x 5), and the two shapes whose backward needs more than 64 KB of LDS (bf16, C = 512, K = 7 and 8).
    Every third case runs without a bias."""
    out = []
    for wi, (dt, C) in enumerate(NARROW + WIDE):
        for gi, geo in enumerate(GEOMETRIES):
            out.append((dt, C, KS[(wi + gi) % len(KS)], geo))
        for K in KS:
            out.append((dt, C, K, GEOMETRIES[1]))
    out.append(("bf16", 512, 7, GEOMETRIES[1]))
    out.append(("bf16", 512, 8, GEOMETRIES[2]))
    seen, cases = set(), []
    for dt, C, K, geo in out:
        if (dt, C, K, geo) in seen:
            continue
        seen.add((dt, C, K, geo))
        cases.append(("%s-C%d-K%d-%dx%dx%d" % ((dt, C, K) + geo), dt, C, K, geo, len(cases) % 3 != 0))
    return cases


def is_wide(dt, C):
    return C // (8 if dt == "bf16" else 4) > 64
