"""Float64 reference of the forward BatchNorm-apply family and the pointwise kernels of the ResNet-50 trunk: one plain
function per C entry point of csrc/pointwise.hip (insar_bn_relu_apply, _pool, _pool_arg, _outc, insar_maxpool2_fwd / _bwd,
insar_colsum, _ld, _partial, insar_scale_f32, insar_mul_dev_f32), csrc/deeplab.hip (insar_conv7x7s2_fwd / _wgrad,
insar_maxpool3s2_fwd / _bwd, insar_bn_add_relu, insar_relu_gate_bwd, insar_sum_hw, insar_broadcast_hw, _gate, insar_dropout)
and csrc/se_residual.hip (insar_se_res_apply: tests/test_se_bottleneck_gpu.py compares it with fp32 torch on the device at
1e-2 for bf16 and never lets a work-group cross an image, so it is NOT yet held per launch and belongs here).

Written from the contracts in include/insar_hip.h and the kernels' header comments, torch on the CPU, no GPU;
tests/test_pointwise_ref_host.py pins every function to an independent torch formulation (F.max_pool2d, F.conv2d, autograd).

Conventions are those of tests/bn_chain_ref.py, whose storage model is reused (`stored` is its round_t: fp32 arithmetic, then
round to nearest even into dtype T): activations are the STORED NHWC tensors [B][H][W][C]. A value function returns
(reference, U): U is the error unit of the rule |got - ref| <= K * 2^-24 * U (sqrt(n) * sum|terms| per sum, a product its own
magnitude, propagated within the launch; an element with U = 0 must match exactly). `dt=torch.float32` evaluates the same
formula in float32 in naive order: the floor from which K is fixed. An exact function returns the one admissible result."""
import math

import torch

from tests.bn_chain_ref import EPS32, F64, _asum, _d, _sum, bf16_half_ulp, f32, ratio, round_t  # noqa: F401

stored = round_t
S2 = math.sqrt(2.0)


def _g(gate, dt):
    return None if gate is None else _d(gate, dt)[:, None, None, :]


# ------------------------------------------------------------------------------------------- BatchNorm apply family
def bn_apply(y, scale, shift, gate, relu, dt=F64):
    """insar_bn_relu_apply (and dst of _pool / _pool_arg): z = relu(y*scale + shift) * gate[n][c], unrounded."""
    yy, sc, sh, g = _d(y, dt), _d(scale, dt), _d(shift, dt), _g(gate, dt)
    p = yy * sc
    a = p + sh
    z = a.clamp_min(0) if relu else a
    out = z * g if g is not None else z
    if dt != F64:
        return out, None
    ua = p.abs() + S2 * (p.abs() + sh.abs())
    if relu:
        ua = ua * (a > 0)
    return out, (ua * g.abs() + out.abs() if g is not None else ua)


def bn_apply_outc(y, scale, shift, gate, relu, wout, bias, T, dt=F64):
    """insar_bn_relu_apply_outc: logits[n][k][h][w] = bias[k] + sum_c round_T(z[c]) * W[k][c]; z is rounded as a stored z would be.
    The unit carries z's own unit through the dot product when T is fp32 (round_T is then the kernel's own rounding)."""
    z, uz = bn_apply(y, scale, shift, gate, relu)
    zr = round_t(z, T).to(dt)
    w = _d(wout, dt)
    terms = zr[:, :, :, None, :] * w[None, None, None]                             # [B][H][W][K][C]
    acc = _sum(terms, 4)
    out = acc + _d(bias, dt) if bias is not None else acc
    out = out.permute(0, 3, 1, 2)
    if dt != F64:
        return out, None
    u = math.sqrt(w.shape[1]) * _asum(terms, 4) + (uz[:, :, :, None, :] * w.abs()[None, None, None]).sum(4)
    if bias is not None:
        u = u + S2 * (acc.abs() + _d(bias).abs())
    return out, u.permute(0, 3, 1, 2)


def bn_add_relu(y, scale, shift, res, relu, dt=F64):
    """insar_bn_add_relu: out = relu(y*scale + shift + res)."""
    yy, sc, sh, r = _d(y, dt), _d(scale, dt), _d(shift, dt), _d(res, dt)
    p = yy * sc
    a = p + sh
    v = a + r
    out = v.clamp_min(0) if relu else v
    if dt != F64:
        return out, None
    u = p.abs() + S2 * (p.abs() + sh.abs()) + S2 * (a.abs() + r.abs())
    return out, (u * (v > 0) if relu else u)


def se_res_apply(y, scale, shift, gate, res, dt=F64):
    """insar_se_res_apply: out = relu(gate[n][c] * (y*scale + shift) + res)."""
    yy, sc, sh, g, r = _d(y, dt), _d(scale, dt), _d(shift, dt), _g(gate, dt), _d(res, dt)
    p = yy * sc
    t = p + sh
    gt = g * t
    v = gt + r
    if dt != F64:
        return v.clamp_min(0), None
    u = g.abs() * (p.abs() + S2 * (p.abs() + sh.abs())) + gt.abs() + S2 * (gt.abs() + r.abs())
    return v.clamp_min(0), u * (v > 0)


# ------------------------------------------------------------------------------------------------------- pools
def _windows2(x):
    B, H, W, C = x.shape
    h2, w2 = H // 2 * 2, W // 2 * 2
    return torch.stack([x[:, 0:h2:2, 0:w2:2], x[:, 0:h2:2, 1:w2:2], x[:, 1:h2:2, 0:w2:2], x[:, 1:h2:2, 1:w2:2]], 0)


def maxpool2(x, last=False):
    """MaxPool2d(2) of the stored x (floor: an odd last row / column belongs to no window). -> (values, arg). The rule: scan
    (0,0), (0,1), (1,0), (1,1); a later element replaces the maximum when it is greater or is NaN (torch's rule), so the
    FIRST maximum wins a tie and a NaN wins. Exact. (`last`: the wrong rule, for the sensitivity test only.)"""
    win = _windows2(x).to(F64)
    best, arg = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.uint8)
    for q in (1, 2, 3):
        take = (win[q] >= best if last else win[q] > best) | torch.isnan(win[q])
        best = torch.where(take, win[q], best)
        arg[take] = q
    return best.to(x.dtype), arg


def maxpool2_bwd(x, dy, dx0, accumulate, T):
    """insar_maxpool2_bwd: dx = round_T((accumulate ? dx0 : 0) + (position == arg ? dy : 0)) inside the windows, dx0 untouched
    outside them. Exact (one fp32 addition of stored values)."""
    B, H, W, C = x.shape
    _, arg = maxpool2(x)
    h2, w2 = H // 2 * 2, W // 2 * 2
    pos = (torch.arange(h2)[:, None] % 2 * 2 + torch.arange(w2)[None, :] % 2)[None, :, :, None]
    up = lambda t: t.repeat_interleave(2, 1).repeat_interleave(2, 2)
    routed = torch.where(up(arg.to(torch.int64)) == pos, up(_d(dy)), torch.zeros(1, dtype=F64))
    out = _d(dx0).clone() if accumulate else torch.zeros(B, H, W, C, dtype=F64)
    out[:, :h2, :w2] = round_t(out[:, :h2, :w2] + routed, T)
    return out


def maxpool3s2(x, clamp_left=False):
    """MaxPool2d(3, stride 2, padding 1) of the stored x -> (values, arg = ky*3 + kx). Padding takes no part; the first
    element inside the image starts the maximum, a later one replaces it when it is greater, or is NaN while the maximum is
    not: first maximum in scan order, the first NaN wins. Exact. (`clamp_left`: column -1 read as column 0, sensitivity only.)"""
    B, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = torch.full((B, 2 * Ho + 1, 2 * Wo + 1, C), float("nan"), dtype=F64)
    ok = torch.zeros(2 * Ho + 1, 2 * Wo + 1, dtype=torch.bool)
    xp[:, 1:H + 1, 1:W + 1], ok[1:H + 1, 1:W + 1] = x.to(F64), True
    if clamp_left:
        xp[:, :, 0], ok[:, 0] = xp[:, :, 1], ok[:, 1]
    m = torch.zeros(B, Ho, Wo, C, dtype=F64)
    arg = torch.full((B, Ho, Wo, C), 255, dtype=torch.uint8)
    for ky in range(3):
        for kx in range(3):
            f = xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
            valid = ok[ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][None, :, :, None]
            take = valid & ((arg == 255) | (f > m) | (torch.isnan(f) & ~torch.isnan(m)))
            m = torch.where(take, f, m)
            arg[take] = ky * 3 + kx
    return m.to(x.dtype), arg


def maxpool3s2_bwd(dy, arg, H, W, T, dt=torch.float32):
    """insar_maxpool3s2_bwd: every input pixel gathers dy of the <= 4 windows whose arg names it, rows then columns ascending,
    added in fp32 (dt; float64 for the host test against autograd) and rounded to T once. Exact in that order."""
    B, Ho, Wo, C = dy.shape
    out = torch.zeros(B, 2 * Ho + 1, 2 * Wo + 1, C, dtype=dt)                          # padded coordinates: pixel (h, w) at (h+1, w+1)
    g = _d(dy, dt)
    for ky, kx in ((2, 2), (2, 0), (2, 1), (0, 2), (0, 0), (0, 1), (1, 2), (1, 0), (1, 1)):
        # ascending window order per pixel: a pixel's lower-numbered window sees it at the HIGHER tap (2 before 0 before 1 is
        # never mixed: an odd coordinate meets taps 2 then 0, an even one tap 1 only)
        v = out[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
        v += torch.where(arg == ky * 3 + kx, g, torch.zeros(1, dtype=dt))
    return round_t(out[:, 1:H + 1, 1:W + 1].to(F64), T)


# ------------------------------------------------------------------------------------------- gates, sums, broadcast
def relu_gate_bwd(dout, out):
    """insar_relu_gate_bwd: g = dout where out > 0 (so not at -0.0, 0.0 or NaN), else +0. Exact."""
    return torch.where(out.to(F64) > 0, dout, torch.zeros_like(dout))


def sum_hw(x, factor, dt=F64):
    """insar_sum_hw: out[n][c] = factor * sum_hw x[n][h][w][c], unrounded."""
    xx = _d(x, dt).reshape(x.shape[0], -1, x.shape[3])
    s = _sum(xx, 1)
    out = s * f32(factor)
    if dt != F64:
        return out, None
    return out, math.sqrt(xx.shape[1]) * _asum(xx, 1) * abs(f32(factor)) + out.abs()


def broadcast_hw(src, dst0, factor, accumulate, gate=None, dt=F64):
    """insar_broadcast_hw / _gate: dst = (accumulate ? dst0 : 0) + factor * src[n][c], then zero where gate is not > 0 (<= 0 or
    NaN). U = 0 (exact) at the zeros and everywhere when nothing is added and factor == 1."""
    s = _d(src, dt)[:, None, None, :] * f32(factor)
    v = s + _d(dst0, dt) if accumulate else s.expand(dst0.shape).clone()
    u = None
    if dt == F64:
        u = (s.abs() + S2 * (s.abs() + _d(dst0).abs())) if accumulate else (s.abs() * (f32(factor) != 1.0)).expand(dst0.shape)
    if gate is not None:
        keep = gate.to(F64) > 0
        v = torch.where(keep, v, torch.zeros(1, dtype=dt))
        u = u * keep if u is not None else None
    return v, u


def dropout_apply(x, mask, p, T):
    """insar_dropout under a given mask: round_T(x * (1 / (1 - p))) where the mask byte is set, +0 elsewhere; the factor is
    formed in fp32 as the host wrapper does. Exact (one fp32 product)."""
    inv = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    return torch.where(mask != 0, (x.float() * inv).to(T), torch.zeros(1, dtype=T))


def colsum(part, accumulate=0, out0=None, dt=F64):
    """insar_colsum / _ld on part[segments][rows][cols] (the gap of an ld > cols already cut away): out[s][c] (+)= sum_r."""
    p = _d(part, dt)
    s = _sum(p, 1)
    out = s + _d(out0, dt) if accumulate else s
    if dt != F64:
        return out, None
    u = math.sqrt(p.shape[1]) * _asum(p, 1)
    return out, (u + S2 * (s.abs() + _d(out0).abs()) if accumulate else u)


def colsum_partial(part, rps, dt=F64):
    """insar_colsum_partial on part[rows][cols]: out[split][c] = sum of rows [split*rps, (split+1)*rps)."""
    rows = part.shape[0]
    v, u = zip(*(colsum(part[None, r0:min(rows, r0 + rps)], dt=dt) for r0 in range(0, rows, rps)))
    return torch.cat(v, 0), (torch.cat(u, 0) if dt == F64 else None)


# ----------------------------------------------------------------------------------------------------- the stem
def _patches(x, T, dt):
    """x [B][H][W] -> round_T(x) gathered as [B][Ho][Wo][49] (tap = ky*7 + kx), zero outside the image."""
    B, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xp = torch.zeros(B, H + 6, W + 6, dtype=dt)
    xp[:, 3:H + 3, 3:W + 3] = round_t(_d(x), T).to(dt)
    return torch.stack([xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] for ky in range(7) for kx in range(7)], 3)


def conv7x7s2(x, w, T, dt=F64):
    """insar_conv7x7s2_fwd: y[n][ho][wo][co] = sum_tap round_T(x) * round_T(w[co][tap]), x [B][H][W] and w [64][49] fp32; the
    kernel rounds both operands to the compute type itself. Unrounded."""
    pt = _patches(x, T, dt)
    wr = round_t(_d(w), T).to(dt)                                                     # [64][49]
    if dt != F64:
        acc = torch.zeros(pt.shape[:3] + (64,), dtype=dt)
        for t in range(49):
            acc = acc + pt[..., t, None] * wr[:, t]
        return acc, None
    y = torch.einsum("bhwt,ct->bhwc", pt, wr)
    return y, 7.0 * torch.einsum("bhwt,ct->bhwc", pt.abs(), wr.abs())


def stem_stats(y_stored, dt=F64):
    """stats[row = n*Ho + ho][2][64] of insar_conv7x7s2_fwd: sum and sum of squares over wo of the STORED y."""
    yy = _d(y_stored, dt).reshape(-1, y_stored.shape[2], 64)
    v = torch.stack([_sum(yy, 1), _sum(yy * yy, 1)], 1)
    if dt != F64:
        return v, None
    rt = math.sqrt(yy.shape[1])
    return v, torch.stack([rt * _asum(yy, 1), (rt + 1) * (yy * yy).sum(1)], 1)


def conv7x7s2_wgrad(x, dy_stored, T, rpb=8, dt=F64):
    """insar_conv7x7s2_wgrad: part[block][co*49 + tap] = sum over the block's `rpb` consecutive output rows (n, ho) and wo of
    dy[co] * round_T(x)[tap]."""
    pt = _patches(x, T, dt)
    B, Ho, Wo, _ = pt.shape
    pt = pt.reshape(B * Ho, Wo, 49)
    g = _d(dy_stored, dt).reshape(B * Ho, Wo, 64)
    vs, us = [], []
    for r0 in range(0, B * Ho, rpb):
        p, q = pt[r0:r0 + rpb].reshape(-1, 49), g[r0:r0 + rpb].reshape(-1, 64)
        if dt != F64:
            acc = torch.zeros(64, 49, dtype=dt)
            for i in range(p.shape[0]):
                acc = acc + q[i][:, None] * p[i][None, :]
            vs.append(acc.reshape(-1))
            continue
        vs.append((q.t() @ p).reshape(-1))
        us.append(math.sqrt(p.shape[0]) * (q.abs().t() @ p.abs()).reshape(-1))
    return torch.stack(vs), (torch.stack(us) if dt == F64 else None)


# ------------------------------------------------------------------------------------------------ bilinear resizes
# insar_bilinear_fwd / _bwd (csrc/deeplab.hip, NCHW fp32) and insar_resize_bilinear_fwd / _bwd (csrc/pointwise.hip, NHWC slices),
# from the formula of the kernels' comment: src = max((o + 1/2) * in / out - 1/2, 0), i0 = floor(src) clamped to in - 1,
# i1 = min(i0 + 1, in - 1), the weight of i1 is the fractional part src - i0. Tensors here are NHWC [B][H][W][C]; the NCHW
# kernels are the same function of a permuted view. `plant` names one deliberate error (tests/test_pointwise_ref_host.py shows
# that the acceptance rule rejects each).
RESIZE_PLANTS = ("i1_unclamped", "scale_inverted", "weights_swapped", "window_short")


def resize_taps(n_out, n_in, dt=F64, plant=None):
    """(i0, i1, l1) of every output index; dt = float32: as the kernels compute them (scale = (float)in / (float)out)."""
    o = torch.arange(n_out, dtype=dt)
    a, b = (n_out, n_in) if plant == "scale_inverted" else (n_in, n_out)
    scale = torch.tensor(float(a), dtype=dt) / torch.tensor(float(b), dtype=dt)
    src = ((o + 0.5) * scale - 0.5).clamp_min(0)
    i0 = src.floor().to(torch.int64).clamp_max(n_in - 1)
    i1 = (i0 + 1) % n_in if plant == "i1_unclamped" else (i0 + 1).clamp_max(n_in - 1)
    l1 = src - i0.to(dt)
    return (i0, i1, 1 - l1) if plant == "weights_swapped" else (i0, i1, l1)


def resize_matrix(n_out, n_in, dt=F64, plant=None):
    """A [n_out][n_in]: row o holds 1 - l1 at i0 and l1 at i1 (their sum where the two coincide)."""
    i0, i1, l1 = resize_taps(n_out, n_in, dt, plant)
    A = torch.zeros(n_out, n_in, dtype=dt)
    rows = torch.arange(n_out)
    A.index_put_((rows, i0), 1 - l1, accumulate=True)
    A.index_put_((rows, i1), l1, accumulate=True)
    return A


def resize_fwd(x, hw_out, dt=F64, plant=None):
    """The resized x [B][Hi][Wi][C] -> [B][Ho][Wo][C], unrounded, and U = sum |w_i * x_i| over the four taps."""
    xx = _d(x, dt)
    h0, h1, lh = resize_taps(hw_out[0], x.shape[1], dt, plant)
    w0, w1, lw = resize_taps(hw_out[1], x.shape[2], dt, plant)
    lh, lw = lh[None, :, None, None], lw[None, None, :, None]

    def blend(v):
        top = (1 - lw) * v[:, h0][:, :, w0] + lw * v[:, h0][:, :, w1]
        bot = (1 - lw) * v[:, h1][:, :, w0] + lw * v[:, h1][:, :, w1]
        return (1 - lh) * top + lh * bot
    if dt != F64:
        return blend(xx), None
    return blend(xx), blend(xx.abs())


def resize_bwd(g, hw_in, dt=F64, plant=None):
    """The adjoint, unrounded: dx[b][i][j][c] = sum_{o, p} Ah[o][i] * Aw[p][j] * g[b][o][p][c], the explicit transpose of
    resize_fwd's weights (no autograd), and U = sqrt(n) * sum |w * g| over the n = (rows with Ah[o][i] != 0) * (columns with
    Aw[p][j] != 0) contributing taps. dt = float32: accumulated tap by tap in raster order of the output."""
    gg = _d(g, dt)
    B, Ho, Wo, Cn = g.shape
    if dt != F64:
        h0, h1, lh = resize_taps(Ho, hw_in[0], dt)
        w0, w1, lw = resize_taps(Wo, hw_in[1], dt)
        dx = torch.zeros(B, hw_in[0], hw_in[1], Cn, dtype=dt)
        for o in range(Ho):
            for hi, wh in ((int(h0[o]), 1 - lh[o]), (int(h1[o]), lh[o])):
                for wi, ww in ((w0, 1 - lw), (w1, lw)):
                    dx[:, hi].index_add_(1, wi, (wh * ww)[None, :, None] * gg[:, o])
        return dx, None
    def fold(v, n_in, dim, taps, count=False):
        """sum over the outputs along `dim` of weight * v into their source indices (the transpose of one resize matrix)."""
        i0, i1, l1 = taps
        shape = [1] * v.dim()
        shape[dim] = -1
        out = torch.zeros(v.shape[:dim] + (n_in,) + v.shape[dim + 1:], dtype=dt)
        for idx, wgt in ((i0, 1 - l1), (i1, l1)):
            out.index_add_(dim, idx, (wgt != 0).to(dt).reshape(shape) * v if count else wgt.reshape(shape) * v)
        return out
    th, tw = resize_taps(Ho, hw_in[0], dt, plant), resize_taps(Wo, hw_in[1], dt, plant)
    if plant == "window_short":                                 # the last output row never reaches the last source row
        i0, i1, l1 = th
        th = (torch.where(i0 == hw_in[0] - 1, 0, i0), torch.where(i1 == hw_in[0] - 1, 0, i1), l1)
        gg = gg.clone()
        gg[:, Ho - 1] = 0
    dx = fold(fold(gg, hw_in[0], 1, th), hw_in[1], 2, tw)
    unit = fold(fold(gg.abs(), hw_in[0], 1, th), hw_in[1], 2, tw)
    # taps per source element: an output whose i0 and i1 coincide counts once
    def ntaps(n_out, n_in, taps):
        i0, i1, l1 = taps
        A = torch.zeros(n_in, dtype=F64)
        A.index_add_(0, i0, ((1 - l1 != 0) | ((i1 == i0) & (l1 != 0))).to(F64))
        A.index_add_(0, i1, ((l1 != 0) & (i1 != i0)).to(F64))
        return A
    n = ntaps(Ho, hw_in[0], th)[:, None] * ntaps(Wo, hw_in[1], tw)[None, :]
    return dx, n.sqrt()[None, :, :, None] * unit


def resize_window(i, n_in, n_out, last_row_clamp=True):
    """[lo, hi]: the output indices the gather-form adjoint kernels visit for source index i, in the kernels' float32
    arithmetic. last_row_clamp = False: without the `if (i == n_in - 1) hi = n_out - 1` line."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    s = f(float(n_in)) / f(float(n_out))
    lo = int(torch.floor((f(float(i)) - 0.5) / s - 0.5)) - 1
    hi = int(torch.ceil((f(float(i)) + 1.5) / s - 0.5)) + 1
    if i == 0:
        lo = 0
    if last_row_clamp and i == n_in - 1:
        hi = n_out - 1
    return max(lo, 0), min(hi, n_out - 1)


# ----------------------------------------------------------------------------------------------- the acceptance rule
def excess(got, ref, unit, K, bf16_out=False):
    """max over the elements of |got - ref| / (2^-24 * U) after the half bf16 ulp a bf16 store may add: accepted iff <= K."""
    got, ref = _d(got).reshape(ref.shape), _d(ref)
    unit = torch.as_tensor(unit, dtype=F64).expand_as(ref)
    if not bf16_out:
        return ratio(got, ref, unit)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    slack = bf16_half_ulp(ref, K * EPS32 * unit)
    return ratio(((got - ref).abs() - slack).clamp_min(0), torch.zeros_like(ref), unit)


def bits_equal(a, b):
    """Bit for bit: -0.0 differs from 0.0; a NaN equals a NaN at the same place (the payload a conversion leaves is not part
    of any contract)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        na, nb = torch.isnan(a), torch.isnan(b)
        if not torch.equal(na, nb):
            return False
        a, b = torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b)
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))
