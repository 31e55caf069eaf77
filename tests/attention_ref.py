"""Float64 reference of the two attention families, one function per kernel launch: SpatialAttention (csrc/spatial_attn.hip)
and the ChannelAttentionModule (csrc/cam.hip).

Plain formulas, written from the contract in include/insar_hip.h ("SpatialAttention", "ChannelAttentionModule") and the
header comments of the two .hip files, torch on the CPU, no GPU. tests/test_attention_ref_host.py pins them to
torch.autograd, which makes them independent of the kernels they judge (tests/test_attention_units_gpu.py).

Conventions: activations are NHWC tensors [B][H][W][C]; the SA maps (z1, z2, s, g2, g1) are [B][H][W], comp and dcomp
[B][H][W][2] (mean, max), both without the halo; bn = (scale1, shift1, mean1, invstd1, scale2, shift2, mean2, invstd2);
w1 (1,2,3,3) and w2 (1,1,3,3) in torch's layout. A row-partitioned pass with `rows` work-groups gives work-group b the
image rows b, b + rows, ... of the B*H rows of the batch; a work-group without rows writes zeros.

Every function takes exactly the tensors its launch reads and returns (values, units), units as in tests/bn_chain_ref.py:
    |got - ref| <= k * 2^-24 * U,
a sum of n terms contributes sqrt(n) * sum|terms|, a product its own magnitude, a cancelling difference its operands', and
an intermediate result formed inside the launch passes its unit on times |d out / d it|. The sigmoid goes through a fast
exponential, whose argument's rounding scales with the argument: U_s = s + s(1-s)(|v| + U_v). A unit of 0 marks an exact
output. `dt=torch.float32` evaluates the same formulas in float32 in naive order (strictly sequential sums); every ReLU
decision is taken in float64 either way, and the folds of sa_bwd_coef stay in float64 as they do on the device (one
rounding to float32 at the end): the floor that fixes k."""
import math

import torch

from tests.bn_chain_ref import F64, _asum, _d, _sum

TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]
SA_PART_COLS = 20


def _shift(t, oy, ox):
    """s[:, h, w] = t[:, h + oy, w + ox], zero where that pixel lies outside the image (t: [B][H][W])."""
    B, H, W = t.shape[:3]
    out = torch.zeros_like(t)
    h0, h1, w0, w1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if h0 < h1 and w0 < w1:
        out[:, h0:h1, w0:w1] = t[:, h0 + oy:h1 + oy, w0 + ox:w1 + ox]
    return out


def _pos(z, scale, shift):
    """(z*scale + shift > 0) in float64, whatever dtype the caller computes in."""
    return _d(z) * float(scale) + float(shift) > 0


def _first_max(t, dim):
    """Maximum along `dim` and the index of its FIRST occurrence; a NaN is the maximum (the first NaN its index)."""
    n = t.shape[dim]
    idx = torch.arange(n).reshape([n if i == dim % t.dim() else 1 for i in range(t.dim())])
    nan = torch.isnan(t)
    anynan = nan.any(dim, keepdim=True)
    m = torch.where(nan, torch.full_like(t, -math.inf), t).amax(dim, keepdim=True)
    hit = torch.where(anynan, nan, t == m)
    arg = torch.where(hit, idx, n).amin(dim)
    m = torch.where(anynan, torch.full_like(m, math.nan), m).squeeze(dim)
    return m, arg


def _block_sums(terms, prop, rows, dt):
    """terms, prop [B][H][W][K] -> value, unit [rows][K] of the row-partitioned sums; prop: the terms' own units."""
    B, H, W, K = terms.shape
    flat, pflat = terms.reshape(B * H, W, K), prop.to(F64).reshape(B * H, W, K)
    val, unit = torch.zeros(rows, K, dtype=dt), torch.zeros(rows, K, dtype=F64)
    for b in range(min(rows, B * H)):
        seg = flat[b::rows].reshape(-1, K)
        val[b] = _sum(seg, 0)
        unit[b] = pflat[b::rows].reshape(-1, K).sum(0) + math.sqrt(seg.shape[0]) * _asum(seg.to(F64), 0)
    return val, unit


def _out(v, u, dt):
    return v, (u if dt == F64 else None)


# ------------------------------------------------------------------------------------------------ SpatialAttention
def sa_compress(x, dt=F64):
    """mean and max over the channels of each pixel, and the first channel holding the maximum."""
    xx, x64 = _d(x, dt), _d(x)
    Cn = xx.shape[3]
    mean = _sum(xx, 3) / float(Cn)
    mx, arg = _first_max(x64, 3)
    zero = torch.zeros_like(mx)
    return _out(dict(mean=mean, max=mx.to(dt), arg=arg),
                dict(mean=math.sqrt(Cn) * _asum(x64, 3) / Cn + mean.abs().to(F64), max=zero, arg=zero), dt)


def _hidden(z1, bn, dt):
    """h1 = ReLU(z1*scale1 + shift1) and its unit."""
    b, z = _d(bn, dt), _d(z1, dt)
    m = _pos(z1, bn[0], bn[1])
    return (z * b[0] + b[1]) * m.to(dt), math.sqrt(2) * ((z * b[0]).abs() + b[1].abs()).to(F64) * m


def sa_conv(which, src, w, bn, rows, training, dt=F64):
    """which 1: z1 = conv(comp, w1), src = comp [B][H][W][2]. which 2: z2 = conv(ReLU(z1*scale1 + shift1), w2), src = z1.
    No bias. stat[rows][2] = (sum z, sum z^2) of each work-group's rows (None in eval: not written)."""
    ww = _d(w, dt).reshape(-1)
    if which == 1:
        c = _d(src, dt)
        terms = [ww[ch * 9 + ky * 3 + kx] * _shift(c[..., ch], ky - 1, kx - 1) for ky, kx in TAPS for ch in (0, 1)]
        prop = torch.zeros(c.shape[:3], dtype=F64)
    else:
        h1, uh = _hidden(src, bn, dt)
        terms = [ww[ky * 3 + kx] * _shift(h1, ky - 1, kx - 1) for ky, kx in TAPS]
        prop = sum(abs(float(ww[ky * 3 + kx])) * _shift(uh, ky - 1, kx - 1) for ky, kx in TAPS)
    t = torch.stack(terms, 0)
    z = _sum(t, 0)
    uz = prop + math.sqrt(len(terms)) * _asum(t.to(F64), 0)
    v, u = dict(z=z, stat=None), dict(z=uz, stat=None)
    if training:
        z64 = z.to(F64)
        v["stat"], u["stat"] = _block_sums(torch.stack([z, z * z], -1), torch.stack([uz, 2 * z64.abs() * uz], -1), rows, dt)
    return _out(v, u, dt)


def sa_gate(x, z2, bn, dt=F64):
    """s = sigmoid(ReLU(z2*scale2 + shift2)), out = x * s (unrounded: the caller allows for the storage dtype)."""
    b, z, xx = _d(bn, dt), _d(z2, dt), _d(x, dt)
    m = _pos(z2, bn[4], bn[5])
    v = (z * b[4] + b[5]) * m.to(dt)
    uv = math.sqrt(2) * ((z * b[4]).abs() + b[5].abs()).to(F64) * m
    s = 1.0 / (1.0 + torch.exp(-v))
    s64 = s.to(F64)
    us = s64 + s64 * (1 - s64) * (v.abs().to(F64) + uv)
    out = xx * s[..., None]
    return _out(dict(s=s, out=out), dict(s=us, out=xx.abs().to(F64) * us[..., None] + out.abs().to(F64)), dt)


def _xhat(z, mean, invstd):
    """(z - mean) * invstd and its unit: a cancelling difference, by its operands' magnitudes."""
    xh = (z - mean) * invstd
    return xh, ((z.abs() + mean.abs()) * invstd.abs() + xh.abs()).to(F64)


def sa_dscale(x, dy, z2, s, bn, rows, dt=F64):
    """g2 = (sum_c dy*x) * s(1-s) * [z2*scale2 + shift2 > 0]; part[rows][0:2] = (sum g2, sum g2 * xhat2)."""
    xx, dd, z, sg, b = _d(x, dt), _d(dy, dt), _d(z2, dt), _d(s, dt), _d(bn, dt)
    prod = dd * xx
    t = _sum(prod, 3)
    ut = math.sqrt(xx.shape[3]) * _asum(prod.to(F64), 3)
    m = _pos(z2, bn[4], bn[5])
    g2 = t * sg * (1 - sg) * m.to(dt)
    ug2 = ((sg * (1 - sg)).abs().to(F64) * ut + math.sqrt(3) * g2.abs().to(F64)) * m
    xh, uxh = _xhat(z, b[6], b[7])
    part, upart = _block_sums(torch.stack([g2, g2 * xh], -1),
                              torch.stack([ug2, ug2 * xh.abs().to(F64) + g2.abs().to(F64) * uxh], -1), rows, dt)
    return _out(dict(g2=g2, part=part), dict(g2=ug2, part=upart), dt)


def sa_bwd_coef(stage, part, count, training, dt=F64):
    """Column folds of part[rows][20] (float64 on the device, rounded once). stage 2: dgamma2, dbeta2, coef = (k1, k2) of BN2;
    stage 1: the same of BN1 plus dw2[9], db2 (columns 2..11); stage 0: dw1[18], db1 (columns 0..18). k = fold / count in
    training, exactly 0 in eval. The unit of a fold is the column's own magnitude."""
    p = _d(part)
    fold, mag = p.sum(0), p.abs().sum(0)
    rnd = lambda t: t.to(dt)
    v, u = {}, {}
    if stage in (1, 2):
        n = str(stage)
        v["dbeta" + n], v["dgamma" + n] = rnd(fold[0]), rnd(fold[1])
        u["dbeta" + n], u["dgamma" + n] = mag[0], mag[1]
        k = fold[:2] / float(count) if training else torch.zeros(2, dtype=F64)
        v["coef"] = rnd(k)
        u["coef"] = mag[:2] / float(count) if training else torch.zeros(2, dtype=F64)
        if stage == 1:
            v["dw2"], v["db2"], u["dw2"], u["db2"] = rnd(fold[2:11]), rnd(fold[11]), mag[2:11], mag[11]
    else:
        v["dw1"], v["db1"], u["dw1"], u["db1"] = rnd(fold[:18]), rnd(fold[18]), mag[:18], mag[18]
    return _out(v, u, dt)


def sa_bwd_stencil(which, g, z, bn, k, w, other, rows, dt=F64):
    """BatchNorm backward on load, dz = scale * (g - k1 - xhat*k2), then the transposed 3x3 stencil.
    which 2: g = g2, z = z2, k = coef[0:2], w = w2, other = z1 -> g1 = conv^T(dz2, w2) * [z1*scale1 + shift1 > 0],
             part[rows][0:12] = (sum g1, sum g1*xhat1, dw2[9], db2).
    which 1: g = g1, z = z1, k = coef[2:4], w = w1, other = comp -> dcomp [B][H][W][2] = conv^T(dz1, w1),
             part[rows][0:19] = (dw1[2][9], db1)."""
    o = 4 if which == 2 else 0
    b, kk, gg, zz, ww = _d(bn, dt), _d(k, dt), _d(g, dt), _d(z, dt), _d(w, dt).reshape(-1)
    sc, mu, inv = b[o], b[o + 2], b[o + 3]
    xh = (zz - mu) * inv
    dz = sc * (gg - kk[0] - xh * kk[1])
    udz = math.sqrt(6) * (sc.abs() * (gg.abs() + kk[0].abs() + (zz.abs() + mu.abs()) * inv.abs() * kk[1].abs())).to(F64)
    dz64 = dz.abs().to(F64)

    def conv_t(ch):            # output pixel q - (ky-1, kx-1) took input q with tap (ky, kx)
        t = torch.stack([ww[ch * 9 + ky * 3 + kx] * _shift(dz, 1 - ky, 1 - kx) for ky, kx in TAPS], 0)
        prop = sum(abs(float(ww[ch * 9 + ky * 3 + kx])) * _shift(udz, 1 - ky, 1 - kx) for ky, kx in TAPS)
        return _sum(t, 0), prop + 3 * _asum(t.to(F64), 0)

    if which == 2:
        cv, ucv = conv_t(0)
        m1 = _pos(other, bn[0], bn[1])
        g1, ug1 = cv * m1.to(dt), ucv * m1
        xh1, uxh1 = _xhat(_d(other, dt), b[2], b[3])
        h1, uh1 = _hidden(other, bn, dt)
        cols = [g1, g1 * xh1] + [dz * _shift(h1, ky - 1, kx - 1) for ky, kx in TAPS] + [dz]
        prop = [ug1, ug1 * xh1.abs().to(F64) + g1.abs().to(F64) * uxh1]
        prop += [udz * _shift(h1, ky - 1, kx - 1).abs().to(F64) + dz64 * _shift(uh1, ky - 1, kx - 1) for ky, kx in TAPS] + [udz]
        v, u = dict(g1=g1), dict(g1=ug1)
    else:
        c = _d(other, dt)
        (d0, u0), (d1, u1) = conv_t(0), conv_t(1)
        cols = [dz * _shift(c[..., ch], ky - 1, kx - 1) for ch in (0, 1) for ky, kx in TAPS] + [dz]
        prop = [udz * _shift(c[..., ch], ky - 1, kx - 1).abs().to(F64) for ch in (0, 1) for ky, kx in TAPS] + [udz]
        v, u = dict(dcomp=torch.stack([d0, d1], -1)), dict(dcomp=torch.stack([u0, u1], -1))
    v["part"], u["part"] = _block_sums(torch.stack(cols, -1), torch.stack(prop, -1), rows, dt)
    return _out(v, u, dt)


def sa_dx(dy, s, dcomp, arg, dt=F64):
    """dx = dy * s + d_mean / C + [c == arg] * d_max (unrounded)."""
    dd, sg, dc = _d(dy, dt), _d(s, dt), _d(dcomp, dt)
    Cn = dd.shape[3]
    dm = dc[..., 0] * torch.tensor(1.0 / Cn, dtype=dt)
    hit = (torch.as_tensor(arg).to(torch.int64)[..., None] == torch.arange(Cn)).to(dt)
    a, c = dd * sg[..., None], hit * dc[..., 1, None]
    dx = a + dm[..., None] + c
    return _out(dx, 2 * (a.abs() + dm.abs()[..., None] + c.abs()).to(F64), dt)


# ------------------------------------------------------------------------------------------------ ChannelAttentionModule
def cam_pool(x, rows_per_part, dt=F64):
    """psum, pmax, parg [B][P][C] over parts of rows_per_part image rows; parg = h*W + w of the first maximum in scan order
    (h, then w). pmax and parg are exact."""
    xx, x64 = _d(x, dt), _d(x)
    B, H, W, Cn = xx.shape
    P = -(-H // rows_per_part)
    psum, upsum = torch.zeros(B, P, Cn, dtype=dt), torch.zeros(B, P, Cn, dtype=F64)
    pmax, parg = torch.zeros(B, P, Cn, dtype=F64), torch.zeros(B, P, Cn, dtype=torch.int64)
    for p in range(P):
        h0, h1 = p * rows_per_part, min(H, (p + 1) * rows_per_part)
        seg = xx[:, h0:h1].reshape(B, -1, Cn)
        psum[:, p] = _sum(seg, 1)
        upsum[:, p] = math.sqrt(seg.shape[1]) * _asum(seg.to(F64), 1)
        m, a = _first_max(x64[:, h0:h1].reshape(B, -1, Cn), 1)
        pmax[:, p], parg[:, p] = m, a + h0 * W
    zero = torch.zeros_like(pmax)
    return _out(dict(psum=psum, pmax=pmax.to(dt), parg=parg), dict(psum=upsum, pmax=zero, parg=zero), dt)


def cam_excite(psum, pmax, parg, w1, w2, H, W, dt=F64):
    """avg = sum_r psum / HW; mx, arg: the first maximum over the parts in order (exact); pre_a = W1 avg, pre_m = W1 mx;
    ha, hm = ReLU of them; gate = sigmoid(W2 (ha + hm))."""
    ps, W1, W2 = _d(psum, dt), _d(w1, dt), _d(w2, dt)
    rows, Cn, Cr = ps.shape[1], ps.shape[2], W1.shape[0]
    avg = _sum(ps, 1) * torch.tensor(1.0 / (float(H) * float(W)), dtype=dt)
    uavg = math.sqrt(rows) * _asum(ps.to(F64), 1) / (H * W) + 2 * avg.abs().to(F64)
    mx64, r = _first_max(_d(pmax), 1)
    arg = torch.as_tensor(parg).to(torch.int64).gather(1, r[:, None, :]).squeeze(1)
    mx = mx64.to(dt)
    ta, tm = W1[None] * avg[:, None, :], W1[None] * mx[:, None, :]
    pa, pm = _sum(ta, 2), _sum(tm, 2)
    upa = (W1.abs().to(F64)[None] * uavg[:, None, :]).sum(2) + math.sqrt(Cn) * _asum(ta.to(F64), 2)
    upm = math.sqrt(Cn) * _asum(tm.to(F64), 2)
    if dt == F64:
        ma, mm = pa > 0, pm > 0
    else:
        ref = cam_excite(psum, pmax, parg, w1, w2, H, W)[0]
        ma, mm = ref["pre_a"] > 0, ref["pre_m"] > 0
    ha, hm = pa * ma.to(dt), pm * mm.to(dt)
    hs = ha + hm
    uhs = upa * ma + upm * mm + hs.abs().to(F64)
    tt = W2[None] * hs[:, None, :]
    t = _sum(tt, 2)
    ut = (W2.abs().to(F64)[None] * uhs[:, None, :]).sum(2) + math.sqrt(Cr) * _asum(tt.to(F64), 2)
    gate = 1.0 / (1.0 + torch.exp(-t))
    g64 = gate.to(F64)
    zero = torch.zeros_like(mx64)
    v = dict(avg=avg, mx=mx, arg=arg, pre_a=pa, pre_m=pm, ha=ha, hm=hm, gate=gate)
    u = dict(avg=uavg, mx=zero, arg=zero, pre_a=upa, pre_m=upm, ha=upa * ma, hm=upm * mm,
             gate=g64 + g64 * (1 - g64) * (t.abs().to(F64) + ut))
    return _out(v, u, dt)


def cam_bwd_coef(red, gate, ha, hm, avg, mx, w1, w2, H, W, dt=F64):
    """red[B][rows][2][C], [.][1][c] = sum_hw dout*x. du = ds * s(1-s); t = W2^T du; dta = t*[ha > 0], dtm = t*[hm > 0];
    coefB = (W1^T dta) / HW, dmax = W1^T dtm; dW2[c][j] = sum_n du * (ha + hm); dW1[j][c] = sum_n dta*avg + dtm*mx."""
    r, s, W1, W2 = _d(red, dt), _d(gate, dt), _d(w1, dt), _d(w2, dt)
    a, m, hA, hM = _d(avg, dt), _d(mx, dt), _d(ha, dt), _d(hm, dt)
    B, rows, _, Cn = r.shape
    Cr = W1.shape[0]
    d = lambda t: t.to(F64)
    ds = _sum(r[:, :, 1], 1)
    uds = math.sqrt(rows) * _asum(d(r[:, :, 1]), 1)
    du = ds * s * (1 - s)
    udu = d((s * (1 - s)).abs()) * uds + math.sqrt(3) * d(du.abs())
    tt = du[:, :, None] * W2[None]                                    # [B][C][Cr]
    t = _sum(tt, 1)
    ut = (udu[:, :, None] * d(W2.abs())[None]).sum(1) + math.sqrt(Cn) * _asum(d(tt), 1)
    ma, mm = _d(ha) > 0, _d(hm) > 0
    dta, dtm = t * ma.to(dt), t * mm.to(dt)
    v, u = dict(du=du, dta=dta, dtm=dtm), dict(du=udu, dta=ut * ma, dtm=ut * mm)
    for name, dh, udh in (("coefB", dta, ut * ma), ("dmax", dtm, ut * mm)):
        tw = dh[:, :, None] * W1[None]                                # [B][Cr][C]
        val = _sum(tw, 1)
        uval = (udh[:, :, None] * d(W1.abs())[None]).sum(1) + math.sqrt(Cr) * _asum(d(tw), 1)
        if name == "coefB":
            val = val * torch.tensor(1.0 / (float(H) * float(W)), dtype=dt)
            uval = uval / (H * W) + 2 * d(val.abs())
        v[name], u[name] = val, uval
    hs = hA + hM
    t2 = du[:, :, None] * hs[:, None, :]                              # [B][C][Cr]
    v["dW2"] = _sum(t2, 0)
    u["dW2"] = (udu[:, :, None] * d(hs.abs())[:, None, :]).sum(0) + d(t2.abs()).sum(0) + math.sqrt(B) * _asum(d(t2), 0)
    t1 = torch.stack([dta[:, :, None] * a[:, None, :], dtm[:, :, None] * m[:, None, :]], 1).reshape(2 * B, Cr, Cn)
    ut1 = torch.stack([(ut * ma)[:, :, None] * d(a.abs())[:, None, :], (ut * mm)[:, :, None] * d(m.abs())[:, None, :]], 1)
    v["dW1"] = _sum(t1, 0)
    u["dW1"] = ut1.reshape(2 * B, Cr, Cn).sum(0) + math.sqrt(2 * B) * _asum(d(t1), 0)
    return _out(v, u, dt)


def cam_scatter_max(dx, dmax, arg, T):
    """dx[n][arg // W][arg % W][c] = round_T(float(old) + dmax[n][c]), every other element bitwise as it was. Exact: the
    sum is formed in float32 and stored as T (T = float64: unrounded, for the host test against autograd)."""
    out = torch.as_tensor(dx).clone()
    B, H, W, Cn = out.shape
    a = torch.as_tensor(arg).to(torch.int64)
    n, c = torch.arange(B)[:, None].expand(B, Cn), torch.arange(Cn)[None, :].expand(B, Cn)
    h, w = a // W, a % W
    if T == F64:
        out[n, h, w, c] = out[n, h, w, c] + _d(dmax)
    else:
        out[n, h, w, c] = (out[n, h, w, c].to(torch.float32) + torch.as_tensor(dmax).to(torch.float32)).to(T)
    return out, torch.zeros(out.shape, dtype=F64)
