"""Float64 reference of the [BatchNorm -> ReLU -> (SE gate)] unit: forward statistics, SE excitation and the backward chain.

Plain formulas, written from the contract in include/insar_hip.h ("BatchNorm2d (+ReLU)", "SELayer", "backward of
[BN -> ReLU -> (SE gate)]", the _pool and _outc forms), torch on the CPU, no GPU. tests/test_bn_chain_ref_host.py pins them to
torch.autograd, which makes them independent of the kernels they judge (tests/test_bn_backward_chain_gpu.py).

Conventions: activations are NHWC tensors [B][H][W][C]; y is the raw (bias-free) conv output;
a = y*scale + shift, mask = (a > 0) when relu else 1, z = relu(a), out = z * gate[n][c].

Every function returns (values, units). `units` has, for each fp32 output, the error unit U of the tolerance rule
    |got - ref| <= k * 2^-24 * U,
a first-order running bound over the float64 values: a sum of n terms contributes sqrt(n) * sum|terms|, a product or a
quotient its own magnitude, and an input that carries a unit of its own passes it on times |d out / d input| — which, for a
cancelling difference such as Q - mean*P, is the propagated term (|Q| + |mean*P|) * invstd. `dt=torch.float32` evaluates the
same formulas in float32 in naive order (strictly sequential sums, no wider accumulator): the floor that fixes k."""
import math

import torch

F64 = torch.float64
EPS32 = 2.0 ** -24


def f32(x):
    """The value a C `float` argument holds."""
    return float(torch.tensor(x, dtype=torch.float32))


def round_t(x, T):
    """x (float64) as it is stored in a tensor of dtype T: through fp32 arithmetic, round to nearest even (T = float64:
    unrounded, for the host test against autograd)."""
    return x if T == F64 else x.to(torch.float32).to(T).to(F64)


def _sum(x, dim):
    if x.dtype == F64:
        return x.sum(dim)
    x = x.movedim(dim, 0)
    acc = torch.zeros_like(x[0])
    for i in range(x.shape[0]):
        acc = acc + x[i]
    return acc


def _asum(x, dim):
    return x.abs().sum(dim)


def _d(x, dt=F64):
    return None if x is None else torch.as_tensor(x).to(dt)


# ------------------------------------------------------------------------------------------------------------------
def finalize(part, count, gamma, beta, conv_bias=None, running_mean=None, running_var=None, num_batches_tracked=None,
             momentum=0.1, eps=1e-5, training=True, dt=F64):
    """part[rows][2][C]: (sum, sum of squares) of y over `count` pixels. -> scale, shift, mean, invstd, running_mean,
    running_var (None when not given), num_batches_tracked."""
    g, b = _d(gamma, dt), _d(beta, dt)
    cb = _d(conv_bias, dt) if conv_bias is not None else torch.zeros_like(g)
    rm, rv = _d(running_mean, dt), _d(running_var, dt)
    v = {"running_mean": rm, "running_var": rv, "num_batches_tracked": num_batches_tracked}
    u = {}
    zero = torch.zeros_like(g, dtype=F64)
    if training:
        p = _d(part, dt)
        rows, n = p.shape[0], float(count)
        s1, s2 = _sum(p[:, 0], 0), _sum(p[:, 1], 0)
        m = s1 / n
        var = (s2 / n - m * m).clamp_min(0)              # a variance is not negative, whatever the rounding of s2 did
        invstd = 1.0 / torch.sqrt(var + eps)
        if rm is not None:
            unbiased = var * n / (n - 1) if n > 1 else var
            v["running_mean"] = (1 - momentum) * rm + momentum * (m + cb)
            v["running_var"] = (1 - momentum) * rv + momentum * unbiased
        if num_batches_tracked is not None:
            v["num_batches_tracked"] = num_batches_tracked + 1
        if dt == F64:
            p64 = p
            um = math.sqrt(rows) * _asum(p64[:, 0], 0) / n + m.abs()
            uvar = math.sqrt(rows) * _asum(p64[:, 1], 0) / n + 2 * m.abs() * um + (s2 / n).abs() + m * m
            uis = 0.5 * invstd ** 3 * uvar + invstd
            if rm is not None:
                f = n / (n - 1) if n > 1 else 1.0
                u["running_mean"] = momentum * um + math.sqrt(3) * (((1 - momentum) * rm).abs() + momentum * (m.abs() + cb.abs()))
                u["running_var"] = momentum * f * uvar + math.sqrt(3) * (((1 - momentum) * rv).abs() + momentum * unbiased.abs())
    else:
        m = rm - cb
        invstd = 1.0 / torch.sqrt(rv + eps)
        if dt == F64:
            um = rm.abs() + cb.abs()
            uis = 2 * invstd
    scale = g * invstd
    shift = b - m * scale
    v.update(scale=scale, shift=shift, mean=m, invstd=invstd)
    if dt == F64:
        us = g.abs() * uis + scale.abs()
        u.update(mean=um, invstd=uis, scale=us,
                 shift=m.abs() * us + scale.abs() * um + math.sqrt(2) * (b.abs() + (m * scale).abs()))
        for k in ("running_mean", "running_var"):
            u.setdefault(k, zero)
    return v, u


def relu_mask(y, scale, shift, relu):
    """(y*scale + shift > 0) in float64, whatever dtype the caller computes in."""
    a = _d(y) * _d(scale) + _d(shift)
    return (a > 0) if relu else torch.ones_like(a, dtype=torch.bool)


def reduce(dout, y, scale, shift, relu, rows_per_part, dt=F64):
    """part[B][P][2][C]: sums over `rows_per_part` image rows of g*mask and g*mask*y (dout None: g = 1, the SE squeeze)."""
    yy = _d(y, dt)
    B, H, W, C = yy.shape
    mask = relu_mask(y, scale, shift, relu).to(dt)
    t0 = mask if dout is None else _d(dout, dt) * mask
    t1 = t0 * yy
    P = -(-H // rows_per_part)
    part = torch.zeros(B, P, 2, C, dtype=dt)
    unit = torch.zeros(B, P, 2, C, dtype=F64)
    for p in range(P):
        h0, h1 = p * rows_per_part, min(H, (p + 1) * rows_per_part)
        for q, t in enumerate((t0, t1)):
            seg = t[:, h0:h1].reshape(B, -1, C)
            part[:, p, q] = _sum(seg, 1)
            unit[:, p, q] = math.sqrt(seg.shape[1]) * _asum(seg.to(F64), 1)
    return part, unit


def se_forward(y, scale, shift, w1, w2, relu=1, part=None, dt=F64):
    """pooled[B][2][C] (sum of mask, of mask*y), sq[B][C] = mean_hw z, hid[B][Cr] = relu(W1 sq), gate = sigmoid(W2 hid).
    part: squeeze slabs [B][P][2][C] to fold instead of y (then y only gives H and W)."""
    B, H, W, C = y.shape
    if part is None:
        part, _ = reduce(None, y, scale, shift, relu, H, dt)
    p = _d(part, dt)
    sc, sh, W1, W2 = _d(scale, dt), _d(shift, dt), _d(w1, dt), _d(w2, dt)
    pooled = _sum(p, 1)
    hw = float(H * W)
    sq = (sc * pooled[:, 1] + sh * pooled[:, 0]) / hw
    pre = _sum(W1[None] * sq[:, None, :], 2)
    hid = pre.clamp_min(0)
    t = _sum(W2[None] * hid[:, None, :], 2)
    gate = 1.0 / (1.0 + torch.exp(-t))
    v = dict(pooled=pooled, sq=sq, hid=hid, gate=gate)
    if dt != F64:
        return v, None
    upool = math.sqrt(p.shape[1]) * _asum(p, 1)
    usq = (sc.abs() * upool[:, 1] + sh.abs() * upool[:, 0]) / hw + math.sqrt(3) * ((sc * pooled[:, 1]).abs() + (sh * pooled[:, 0]).abs()) / hw
    uhid = (W1.abs()[None] * usq[:, None, :]).sum(2) + math.sqrt(C) * _asum(W1[None] * sq[:, None, :], 2)
    ut = (W2.abs()[None] * uhid[:, None, :]).sum(2) + math.sqrt(W1.shape[0]) * _asum(W2[None] * hid[:, None, :], 2)
    # the sigmoid through a fast exponential: the argument's rounding scales with |t|, exp, 1 + e and the division add a few ulp
    ugate = gate * (1 - gate) * ut + gate * (4 + t.abs())
    return v, dict(pooled=upool, sq=usq, hid=uhid, gate=ugate)


def coef(red, H, W, scale, shift, mean, invstd, training, use_se=0, pooled=None, sq=None, hid=None, gate=None, w1=None,
         w2=None, dt=F64):
    """red[B][rows][2][C] (folded per image here). -> dgamma, dbeta, k1, k2, dconv_bias, tb, tg ([B][C] per-image parts of
    dbeta / dgamma) and, with use_se, coefB[B][C], dW1 (Cr, C), dW2 (C, Cr)."""
    r = _d(red, dt)
    B, rows, _, C = r.shape
    sc, sh, mu, istd = _d(scale, dt), _d(shift, dt), _d(mean, dt), _d(invstd, dt)
    hw, N = float(H * W), float(B * H * W)
    P2, Q = _sum(r[:, :, 0], 1), _sum(r[:, :, 1], 1)
    uP, uQ = math.sqrt(rows) * _asum(r[:, :, 0].to(F64), 1), math.sqrt(rows) * _asum(r[:, :, 1].to(F64), 1)
    p4 = istd * (Q - mu * P2)
    up4 = istd.abs() * (uQ + mu.abs() * uP) + math.sqrt(3) * istd.abs() * (Q.abs() + (mu * P2).abs())
    v, u = {}, {}
    if use_se:
        s, W1, W2, hd, sqq, pl = _d(gate, dt), _d(w1, dt), _d(w2, dt), _d(hid, dt), _d(sq, dt), _d(pooled, dt)
        Cr = W1.shape[0]
        ds = sc * Q + sh * P2                                     # sum_hw dout * z
        du = ds * s * (1 - s)
        dtp = _sum(du[:, :, None] * W2[None], 1) * (hd > 0).to(dt)    # [B][Cr]
        dsq = _sum(dtp[:, :, None] * W1[None], 1)                  # [B][C]
        cb = dsq / hw
        cnt, sy = pl[:, 0], pl[:, 1]
        p5 = istd * (sy - mu * cnt)
        tb = s * P2 + cb * cnt
        tg = s * p4 + cb * p5
        v.update(coefB=cb, dW2=_sum(du[:, :, None] * hd[:, None, :], 0), dW1=_sum(dtp[:, :, None] * sqq[:, None, :], 0))
        uds = sc.abs() * uQ + sh.abs() * uP + math.sqrt(2) * ((sc * Q).abs() + (sh * P2).abs())
        udu = (s * (1 - s)).abs() * uds + math.sqrt(3) * du.abs()
        udt = ((udu[:, :, None] * W2.abs()[None]).sum(1) + math.sqrt(C) * _asum(du[:, :, None] * W2[None], 1)) * (hd > 0)
        udsq = (udt[:, :, None] * W1.abs()[None]).sum(1) + math.sqrt(Cr) * _asum(dtp[:, :, None] * W1[None], 1)
        ucb = udsq / hw + 2 * cb.abs()
        up5 = math.sqrt(3) * istd.abs() * (sy.abs() + (mu * cnt).abs())
        utb = s.abs() * uP + cnt.abs() * ucb + math.sqrt(2) * ((s * P2).abs() + (cb * cnt).abs())
        utg = s.abs() * up4 + p5.abs() * ucb + cb.abs() * up5 + math.sqrt(2) * ((s * p4).abs() + (cb * p5).abs())
        u.update(coefB=ucb,
                 dW2=(udu[:, :, None] * hd.abs()[:, None, :]).sum(0) + math.sqrt(B) * _asum(du[:, :, None] * hd[:, None, :], 0),
                 dW1=(udt[:, :, None] * sqq.abs()[:, None, :]).sum(0) + math.sqrt(B) * _asum(dtp[:, :, None] * sqq[:, None, :], 0))
    else:
        tb, tg, utb, utg = P2, p4, uP, up4
    db, dg = _sum(tb, 0), _sum(tg, 0)
    udb = utb.sum(0) + math.sqrt(B) * _asum(tb, 0)
    udg = utg.sum(0) + math.sqrt(B) * _asum(tg, 0)
    zero = torch.zeros_like(db)
    v.update(dbeta=db, dgamma=dg, tb=tb, tg=tg, k1=db / N if training else zero, k2=dg / N if training else zero,
             dconv_bias=zero if training else sc * db)
    u.update(dbeta=udb, dgamma=udg, tb=utb, tg=utg, k1=(udb / N + 2 * (db / N).abs()) if training else zero.to(F64),
             k2=(udg / N + 2 * (dg / N).abs()) if training else zero.to(F64),
             dconv_bias=zero.to(F64) if training else sc.abs() * udb + (sc * db).abs())
    return v, (u if dt == F64 else None)


def apply(dout, y, scale, shift, mean, invstd, relu, gate=None, coefB=None, k1=None, k2=None, tb=None, tg=None, dt=F64):
    """dy = scale * ((dout*gate + coefB) * mask - k1 - xhat*k2), xhat = (y - mean) * invstd. k1 / k2 given, or folded from
    the per-image parts tb / tg [B][C] (the _part form: k = sum_n t[n] / (B*H*W))."""
    g, yy = _d(dout, dt), _d(y, dt)
    B, H, W, C = yy.shape
    sc, mu, istd = _d(scale, dt), _d(mean, dt), _d(invstd, dt)
    mask = relu_mask(y, scale, shift, relu).to(dt)
    N = float(B * H * W)
    if tb is not None:
        tb_, tg_ = _d(tb, dt), _d(tg, dt)
        k1_, k2_ = _sum(tb_, 0) / N, _sum(tg_, 0) / N
        uk1 = math.sqrt(B) * _asum(tb_, 0) / N + 2 * k1_.abs()
        uk2 = math.sqrt(B) * _asum(tg_, 0) / N + 2 * k2_.abs()
    else:
        k1_, k2_ = _d(k1, dt), _d(k2, dt)
        uk1 = uk2 = torch.zeros(C, dtype=F64)
    s = _d(gate, dt)[:, None, None, :] if gate is not None else torch.ones(1, dtype=dt)
    cb = _d(coefB, dt)[:, None, None, :] if coefB is not None else torch.zeros(1, dtype=dt)
    xhat = (yy - mu) * istd
    dy = sc * ((g * s + cb) * mask - k1_ - xhat * k2_)
    if dt != F64:
        return dy, None
    # xhat is a cancelling difference when |mean| >> sigma: its propagated term is (|y| + |mean|) * invstd
    unit = sc.abs() * (uk1 + xhat.abs() * uk2) + math.sqrt(6) * sc.abs() * (
        ((g * s).abs() + cb.abs()) * mask + k1_.abs() + (yy.abs() + mu.abs()) * istd.abs() * k2_.abs())
    return dy, unit


# ------------------------------------------------------------------------------------------------------------------
def pool_arg(z):
    """Arg-max map of MaxPool2d(2) over stored z [B][H][W][C]: 2*(row parity) + (column parity) of the FIRST maximum in
    scan order (0,0), (0,1), (1,0), (1,1)."""
    B, H, W, C = z.shape
    win = torch.stack([z[:, 0::2, 0::2], z[:, 0::2, 1::2], z[:, 1::2, 0::2], z[:, 1::2, 1::2]], 0).to(F64)
    best, arg = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.uint8)
    for p in (1, 2, 3):
        better = win[p] > best
        best = torch.where(better, win[p], best)
        arg[better] = p
    return arg


def pool_dout(dskip, dpooled, arg, T):
    """round_T(dskip + (arg == position ? dpooled : 0)) at full resolution."""
    B, H, W, C = dskip.shape
    hh = torch.arange(H)[:, None] % 2 * 2 + torch.arange(W)[None, :] % 2                  # position of (h, w) in its window
    up = lambda t: t.repeat_interleave(2, 1).repeat_interleave(2, 2)
    hit = up(arg.to(torch.int64)) == hh[None, :, :, None]
    return round_t(_d(dskip) + torch.where(hit, up(_d(dpooled)), torch.zeros(1, dtype=F64)), T)


def outc_dout(dlogits, wout, T):
    """round_T(sum_k dlogits[n][k][h][w] * W[k][c]) as [B][H][W][C], and its fp32 unit (sum of K products)."""
    dl, w = _d(dlogits), _d(wout)
    terms = dl.permute(0, 2, 3, 1)[..., None] * w[None, None, None]                          # [B][H][W][K][C]
    return round_t(terms.sum(3), T), math.sqrt(w.shape[0]) * terms.abs().sum(3)


def outc_wpart(dlogits, wout_shape, y, scale, shift, gate, relu, rows_per_part, T):
    """The output conv's parameter-gradient partials of every row part: wpart[B*P][K*C + K] =
    (sum dlogits[k] * z[c], sum dlogits[k]), z = round_T(relu(y*scale + shift) * gate[n])."""
    dl = _d(dlogits)
    yy = _d(y)
    B, H, W, C = yy.shape
    K = wout_shape[0]
    a = yy * _d(scale) + _d(shift)
    z = a.clamp_min(0) if relu else a
    if gate is not None:
        z = z * _d(gate)[:, None, None, :]
    z = round_t(z, T)
    P = -(-H // rows_per_part)
    part = torch.zeros(B, P, K * C + K, dtype=F64)
    unit = torch.zeros_like(part)
    for p in range(P):
        h0, h1 = p * rows_per_part, min(H, (p + 1) * rows_per_part)
        n = (h1 - h0) * W
        d = dl[:, :, h0:h1].reshape(B, K, n)
        zz = z[:, h0:h1].reshape(B, n, C)
        t = d[:, :, :, None] * zz[:, None, :, :]                                             # [B][K][n][C]
        part[:, p, :K * C] = t.sum(2).reshape(B, K * C)
        unit[:, p, :K * C] = math.sqrt(n) * t.abs().sum(2).reshape(B, K * C)
        part[:, p, K * C:] = d.sum(2)
        unit[:, p, K * C:] = math.sqrt(n) * d.abs().sum(2)
    return part.reshape(B * P, -1), unit.reshape(B * P, -1)


# ------------------------------------------------------------------------------------------------------------------
def bf16_half_ulp(ref, slack):
    """Half a bf16 ulp of the reference value (of |ref| + slack, so that a value the fp32 error carries across a binade
    boundary is covered)."""
    mag = (ref.abs() + slack).clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(mag)) - 8)


def ratio(got, ref, unit):
    """max over the elements of |got - ref| / (2^-24 * unit): the figure the tolerance rule bounds by k. An element whose
    unit is 0 (an exact output) must match exactly: inf otherwise."""
    err = (_d(got) - _d(ref)).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    unit = torch.as_tensor(unit, dtype=F64).expand_as(err)
    r = torch.where(unit > 0, err / (EPS32 * unit.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0
