"""Reference statement of the generic weight-gradient path (pixel tables, split-K slabs, fold, reduce, column sums) and of
ConvTranspose2d(k=2, s=2) with its three gradients, written from include/insar_hip.h — not from the kernels — in plain
torch float64 / int64 (tables, slabs, folds and column sums on the CPU; the transposed conv on its operands' device, so
that the larger GPU cases need not cross to the host). tests/test_wgrad_ref_host.py holds it to torch.autograd; the GPU
tests (test_wgrad_generic_gpu.py, test_conv_transpose_gpu.py) hold the kernels to it.

Buffers. An activation is a padded NHWC buffer [B][H+2][W+2][C] with a one-pixel zero halo; a "padded pixel index" is the
row of that buffer flattened to [B*(H+2)*(W+2)][C]: pixel (n, h, w) of the interior is row (n*(H+2) + h + 1)*(W+2) + w + 1,
row 0 is the halo corner of image 0.

The in-bounds rule of pixel_table_taps. The header says of the per-tap tables only "out-of-bounds -> pixel 0". What counts
as in bounds is settled by the caller (deeplab.ConvUnit: a tap is out of bounds when `off < -1 or (n_out-1)*s + off > n_in`,
and only then is INSAR_IGEMM_OOB_ZERO set, whose own text says "the 1-pixel halo covers only |dy|,|dx| <= 1"): a position is
in bounds while it lies inside the PADDED buffer, i.e. interior coordinates -1 .. Hb and -1 .. Wb. A tap that lands on the
one-pixel halo keeps the halo pixel's own index (it reads the zeros stored there); only positions beyond the halo, which
would alias another row or image, get entry 0. Entries p >= B*H*W are 0 as well.

Exactness. Every function takes int64 or float64 tensors. int64 operands are contracted in float64 — exact while every
partial sum stays below 2^53, which is asserted — and returned as int64, so that a kernel fed the same small integers in
bf16 / fp32 has one right answer whatever its summation order."""
import torch

WG_BKP = 64          # pixels per K step (include/insar_hip.h: Mpad is a multiple of 64)


def round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


# ---- pixel tables -------------------------------------------------------------------------------------------------------
def pixel_table(B, H, W, s, Hb, Wb, tail, Mpad):
    """tab[p] = (n*(Hb+2) + h*s + 1)*(Wb+2) + w*s + 1 for p = (n*H + h)*W + w < B*H*W; `tail` beyond. int64 [Mpad]."""
    assert Mpad >= B * H * W
    tab = torch.full((Mpad,), int(tail), dtype=torch.int64)
    p = 0
    for n in range(B):
        for h in range(H):
            for w in range(W):
                tab[p] = (n * (Hb + 2) + h * s + 1) * (Wb + 2) + w * s + 1
                p += 1
    return tab


def pixel_table_taps(B, H, W, s, Hb, Wb, taps, Mpad):
    """tab[t][p] = padded pixel index of (n, h*s + dy_t, w*s + dx_t) in a (Hb, Wb) buffer while that position lies inside
    the padded buffer (the halo included, see the module docstring); 0 otherwise and for p >= B*H*W. int64 [ntaps][Mpad]."""
    assert Mpad >= B * H * W
    tab = torch.zeros((len(taps), Mpad), dtype=torch.int64)
    for t, (dy, dx) in enumerate(taps):
        p = 0
        for n in range(B):
            for h in range(H):
                for w in range(W):
                    hh, ww = h * s + dy, w * s + dx
                    if -1 <= hh <= Hb and -1 <= ww <= Wb:
                        tab[t, p] = (n * (Hb + 2) + hh + 1) * (Wb + 2) + ww + 1
                    p += 1
    return tab


def pad_nhwc(t_nchw):
    """NCHW interior -> the flattened padded NHWC buffer [B*(H+2)*(W+2)][C] with a zero halo."""
    B, C, H, W = t_nchw.shape
    buf = torch.zeros((B, H + 2, W + 2, C), dtype=t_nchw.dtype)
    buf[:, 1:-1, 1:-1] = t_nchw.permute(0, 2, 3, 1)
    return buf.reshape(-1, C)


# ---- split-K slabs, fold, reduce ----------------------------------------------------------------------------------------
def _contract(y, x):
    """y[p][co], x[p][ci] -> [co][ci] = sum_p y*x; int64 operands exactly (through float64, bounded below 2^53)."""
    if y.dtype == torch.int64:
        assert x.dtype == torch.int64
        bound = float(y.abs().max()) * float(x.abs().max()) * max(1, y.shape[0]) if y.numel() and x.numel() else 0.0
        assert bound < 2.0 ** 53
        return (y.double().t() @ x.double()).to(torch.int64)
    assert y.dtype == torch.float64 and x.dtype == torch.float64
    return y.t() @ x


def wgrad_slabs(x_padded, dy_padded, tabx, tabdy, offx, offdy, nsplit, tabx_tap_stride=0):
    """part[split][tap][co][ci] = sum_{p in split} dy[tabdy[p] + offdy[tap], co] * x[tabx_tap[p] + offx[tap], ci].

    x_padded [pixels][Cin], dy_padded [pixels][Cout]: flattened padded buffers (the channel slice already taken).
    tabdy int64 [Mpad]; tabx int64 [Mpad], or with tabx_tap_stride != 0 the flat per-tap tables, tap t at
    tabx[t*tabx_tap_stride : t*tabx_tap_stride + Mpad]. A K step is 64 consecutive p; with ksteps = Mpad / 64, split s owns
    K steps [s*ceil(ksteps/nsplit), (s+1)*ceil(ksteps/nsplit)) clipped to ksteps; a split with no step is all zeros."""
    Mpad = tabdy.numel()
    assert Mpad >= WG_BKP and Mpad % WG_BKP == 0 and nsplit >= 1 and len(offx) == len(offdy)
    ntaps = len(offx)
    ksteps = Mpad // WG_BKP
    sps = -(-ksteps // nsplit)
    cin, cout = x_padded.shape[1], dy_padded.shape[1]
    part = torch.zeros((nsplit, ntaps, cout, cin), dtype=x_padded.dtype)
    for s in range(nsplit):
        k0, k1 = min(s * sps, ksteps), min((s + 1) * sps, ksteps)
        if k0 >= k1:
            continue
        rows = slice(k0 * WG_BKP, k1 * WG_BKP)
        for t in range(ntaps):
            tx = tabx[t * tabx_tap_stride: t * tabx_tap_stride + Mpad] if tabx_tap_stride else tabx
            ix, iy = tx[rows] + int(offx[t]), tabdy[rows] + int(offdy[t])
            assert int(ix.min()) >= 0 and int(ix.max()) < x_padded.shape[0]
            assert int(iy.min()) >= 0 and int(iy.max()) < dy_padded.shape[0]
            part[s, t] = _contract(dy_padded[iy], x_padded[ix])
    return part


def fold(part, group):
    """part_out[g] = sum of the `group` consecutive slabs part[g*group : (g+1)*group] (the last group may be short)."""
    nsplit = part.shape[0]
    return torch.stack([part[g:g + group].sum(0) for g in range(0, nsplit, group)])


def reduce(part, layout, accumulate_into=None):
    """grad = sum_split part[split][tap][co][ci], re-laid out: layout 0 (Conv2d) grad[co][ci][tap], layout 1
    (ConvTranspose2d) grad[ci][co][tap]; added to `accumulate_into` (same layout) when given."""
    assert layout in (0, 1)
    g = part.sum(0)                                              # [tap][co][ci]
    g = g.permute(1, 2, 0) if layout == 0 else g.permute(2, 1, 0)
    g = g.contiguous()
    return g if accumulate_into is None else accumulate_into + g


def colsum(part, segments, rows, cols, ld=None, accumulate_into=None):
    """out[s][c] = sum_r part[(s*rows + r)*ld + c] over the flat tensor `part` (ld = cols when None)."""
    ld = cols if ld is None else ld
    assert ld >= cols
    need = ((segments * rows - 1) * ld + cols)
    view = torch.zeros(segments * rows * ld, dtype=part.dtype)
    view[:need] = part.reshape(-1)[:need]
    out = view.reshape(segments, rows, ld)[:, :, :cols].sum(1)
    return out if accumulate_into is None else accumulate_into + out


def colsum_partial(part, rows, cols, rps):
    """out[i][c] = sum of rows [i*rps, (i+1)*rps) (clipped to `rows`) of part[rows][cols]."""
    p = part.reshape(rows, cols)
    return torch.stack([p[r:r + rps].sum(0) for r in range(0, rows, rps)])


# ---- ConvTranspose2d(k=2, s=2) ---------------------------------------------------------------------------------------------
TAPS2 = [(a, b) for a in range(2) for b in range(2)]


def conv_transpose_k2s2(x, w, bias=None):
    """out[n, co, 2i+a, 2j+b] = sum_ci x[n, ci, i, j] * w[ci, co, a, b] (+ bias[co]); x [B][Ci][h][w], w [Ci][Co][2][2]."""
    B, ci, h, wd = x.shape
    co = w.shape[1]
    out = torch.zeros((B, co, 2 * h, 2 * wd), dtype=x.dtype, device=x.device)
    xp = x.permute(0, 2, 3, 1).reshape(-1, ci)                   # [pixel][ci]
    for a, b in TAPS2:
        v = _mm(xp, w[:, :, a, b]).reshape(B, h, wd, co).permute(0, 3, 1, 2)
        out[:, :, a::2, b::2] = v
    if bias is not None:
        out = out + bias.reshape(1, co, 1, 1)
    return out


def conv_transpose_k2s2_backward(x, w, dout):
    """(dx, dw, dbias) of conv_transpose_k2s2 for the upstream gradient dout [B][Co][2h][2w]:
    dx[n, ci, i, j] = sum_{co,a,b} dout[n, co, 2i+a, 2j+b] * w[ci, co, a, b]
    dw[ci, co, a, b] = sum_{n,i,j} x[n, ci, i, j] * dout[n, co, 2i+a, 2j+b];   dbias[co] = sum_{n,y,x} dout[n, co, y, x]."""
    B, ci, h, wd = x.shape
    co = w.shape[1]
    xp = x.permute(0, 2, 3, 1).reshape(-1, ci)
    dx = torch.zeros((B * h * wd, ci), dtype=x.dtype, device=x.device)
    dw = torch.zeros_like(w)
    for a, b in TAPS2:
        g = dout[:, :, a::2, b::2].permute(0, 2, 3, 1).reshape(-1, co)      # [pixel][co]
        dx = dx + _mm(g, w[:, :, a, b].t())
        dw[:, :, a, b] = _mm(xp.t(), g)
    return dx.reshape(B, h, wd, ci).permute(0, 3, 1, 2).contiguous(), dw, dout.sum((0, 2, 3))


def _mm(a, b):
    if a.dtype == torch.int64:
        bound = float(a.abs().max()) * float(b.abs().max()) * a.shape[1] if a.numel() and b.numel() else 0.0
        assert b.dtype == torch.int64 and bound < 2.0 ** 53
        return (a.double() @ b.double()).to(torch.int64)
    assert a.dtype == torch.float64 and b.dtype == torch.float64
    return a @ b
