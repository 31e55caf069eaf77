"""Reference statement of the 3x3 convolution family (forward, input gradient, per-channel BatchNorm statistics), written
from include/insar_hip.h — not from the kernels — in plain torch int64 / float64, on its operands' device (so that the
larger GPU cases need not cross to the host), and the integer operand recipe under which a kernel that accumulates in fp32
and stores bf16 has ONE right answer whatever its tiling, summation order or rounding mode. tests/test_conv_ref_host.py
holds it to torch.nn.functional and to autograd; tests/test_conv3x3_exact_gpu.py holds the kernels to it.

The operation. x [B][Ci][H][W], w [Co][Ci][3][3], dilation d >= 1, padding d, stride s in {1, 2}:
    y[n, co, oy, ox] = sum_{ci, ky, kx} x[n, ci, oy*s + (ky-1)*d, ox*s + (kx-1)*d] * w[co, ci, ky, kx]   (zero outside x)
with Ho = (H - 1) // s + 1, Wo = (W - 1) // s + 1, and for an upstream gradient g [B][Co][Ho][Wo]
    dx[n, ci, iy, ix] = sum over (co, ky, kx, oy, ox) with oy*s + (ky-1)*d == iy, ox*s + (kx-1)*d == ix of g * w.
The statistics of y are (sum_{n,oy,ox} y, sum_{n,oy,ox} y^2) per channel.

Exactness. Every function takes int64 or float64 tensors. int64 operands are contracted in float64 — exact while every
partial sum stays below 2^53, which is asserted — and returned as int64."""
from types import SimpleNamespace

import torch

OUT_LIMIT = 256          # |v| <= 256: an integer that bf16 (8 significant bits) holds exactly, under any rounding mode
SUM_LIMIT = 2 ** 24      # integers below 2^24 in magnitude: every fp32 partial sum of them, in any partition, is exact


def _mm(a, b):
    """a [m][k] @ b [k][n]; int64 operands exactly (through float64, bounded below 2^53)."""
    if a.dtype == torch.int64:
        bound = float(a.abs().max()) * float(b.abs().max()) * a.shape[1] if a.numel() and b.numel() else 0.0
        assert b.dtype == torch.int64 and bound < 2.0 ** 53
        return (a.double() @ b.double()).to(torch.int64)
    assert a.dtype == torch.float64 and b.dtype == torch.float64
    return a @ b


def out_size(n: int, stride: int) -> int:
    return (n - 1) // stride + 1


def conv3x3(x, w, dil: int = 1, stride: int = 1, bias=None):
    """y of the module docstring (+ bias[co]); x [B][Ci][H][W], w [Co][Ci][3][3] -> [B][Co][Ho][Wo]."""
    assert stride in (1, 2) and dil >= 1 and tuple(w.shape[2:]) == (3, 3) and w.shape[1] == x.shape[1]
    B, ci, H, W = x.shape
    co = w.shape[0]
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xp = torch.zeros((B, H + 2 * dil, W + 2 * dil, ci), dtype=x.dtype, device=x.device)       # NHWC with a zero border
    xp[:, dil:dil + H, dil:dil + W] = x.permute(0, 2, 3, 1)
    out = torch.zeros((B * Ho * Wo, co), dtype=x.dtype, device=x.device)
    for ky in range(3):
        for kx in range(3):
            y0, x0 = ky * dil, kx * dil                         # (ky-1)*d in x = ky*d in xp
            v = xp[:, y0:y0 + (Ho - 1) * stride + 1:stride, x0:x0 + (Wo - 1) * stride + 1:stride]
            out = out + _mm(v.reshape(-1, ci), w[:, :, ky, kx].t().contiguous())
    out = out.reshape(B, Ho, Wo, co).permute(0, 3, 1, 2).contiguous()
    return out if bias is None else out + bias.reshape(1, co, 1, 1)


def conv3x3_input_grad(g, w, hw, dil: int = 1, stride: int = 1):
    """dx of the module docstring for the input extent hw = (H, W); g [B][Co][Ho][Wo], w [Co][Ci][3][3] -> [B][Ci][H][W]."""
    assert stride in (1, 2) and dil >= 1 and tuple(w.shape[2:]) == (3, 3) and w.shape[0] == g.shape[1]
    H, W = hw
    B, co, Ho, Wo = g.shape
    assert (Ho, Wo) == (out_size(H, stride), out_size(W, stride))
    ci = w.shape[1]
    dxp = torch.zeros((B, H + 2 * dil, W + 2 * dil, ci), dtype=g.dtype, device=g.device)
    gp = g.permute(0, 2, 3, 1).reshape(-1, co)
    for ky in range(3):
        for kx in range(3):
            y0, x0 = ky * dil, kx * dil
            v = _mm(gp, w[:, :, ky, kx].contiguous()).reshape(B, Ho, Wo, ci)
            dxp[:, y0:y0 + (Ho - 1) * stride + 1:stride, x0:x0 + (Wo - 1) * stride + 1:stride] += v
    return dxp[:, dil:dil + H, dil:dil + W].permute(0, 3, 1, 2).contiguous()


def channel_stats(y):
    """(sum y, sum y^2) over batch and pixels, per channel: two [C] tensors of y's dtype."""
    return y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))


def weight_keep_probability(cin: int, cout: int) -> float:
    return min(1.0, 16.0 / max(cin, cout))


def _ints(gen, shape, lo=-1, hi=1):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64)


def integer_operands(seed: int, B: int, cin: int, cout: int, H: int, W: int, dil: int = 1, stride: int = 1, device="cpu",
                     q=None, lo: int = -1, hi: int = 1):
    """Seeded integer operands of one convolution with its reference results, all int64 on `device`:
    x [B][cin][H][W] and g [B][cout][Ho][Wo] uniform in {-1, 0, 1} (lo .. hi); w [cout][cin][3][3] uniform in {-1, 0, 1},
    each element kept with probability q (default min(1, 16 / max(cin, cout))) and zero otherwise; y = conv3x3(x, w), dx =
    conv3x3_input_grad(g, w), (s1, s2) = channel_stats(y). Drawn on the CPU generator: the same values on every device.

    Asserts what makes a bf16 / fp32 kernel's result unique: |y|, |dx| <= OUT_LIMIT, and per channel sum |y| < SUM_LIMIT,
    sum y^2 < SUM_LIMIT."""
    gen = torch.Generator().manual_seed(seed)
    q = weight_keep_probability(cin, cout) if q is None else q
    x = _ints(gen, (B, cin, H, W), lo, hi)
    w = _ints(gen, (cout, cin, 3, 3)) * (torch.rand((cout, cin, 3, 3), generator=gen) < q).to(torch.int64)
    g = _ints(gen, (B, cout, out_size(H, stride), out_size(W, stride)), lo, hi)
    x, w, g = x.to(device), w.to(device), g.to(device)
    y = conv3x3(x, w, dil, stride)
    dx = conv3x3_input_grad(g, w, (H, W), dil, stride)
    s1, s2 = channel_stats(y)
    assert_exact_in_bf16(y, dx)
    assert_sums_exact_in_fp32(y)
    return SimpleNamespace(x=x, w=w, g=g, y=y, dx=dx, s1=s1, s2=s2, dil=dil, stride=stride)


def assert_exact_in_bf16(*tensors):
    for t in tensors:
        assert t.dtype == torch.int64 and int(t.abs().max()) <= OUT_LIMIT, int(t.abs().max())


def assert_sums_exact_in_fp32(y):
    assert y.dtype == torch.int64
    assert int(y.abs().sum((0, 2, 3)).max()) < SUM_LIMIT and int((y * y).sum((0, 2, 3)).max()) < SUM_LIMIT


# ---- the layers of tests/test_switch_routes_gpu.py ----------------------------------------------------------------------------------
# (Cin, Cout, (B, H, W)). The GPU cases find their batches from the library's queries and the device's CU count and refuse a
# shape that is not listed here (these are the ones of a 256-CU device); tests/test_conv_ref_host.py asserts the exactness
# bounds of each.
SWITCH_SEED = 4242
SWITCH_ROUTE_LAYERS = [(64, 64, (3, 30, 30)), (128, 128, (2, 16, 32)), (64, 128, (4, 128, 128)), (128, 256, (4, 128, 128)),
                       (256, 256, (2, 60, 72)), (64, 256, (4, 128, 130))]


def consumer_sums(dx, yv, scale, shift):
    """(sum dx * mask, sum dx * mask * yv) per channel, mask = [scale * yv + shift > 0] (InsarBstat, include/insar_hip.h): the
    BatchNorm-backward sums a producer GEMM writes for the unit that consumes dx. Asserts the bound under which fp32 holds
    every partial sum exactly."""
    mask = (scale.reshape(1, -1, 1, 1) * yv + shift.reshape(1, -1, 1, 1) > 0).to(torch.int64)
    assert bool(mask.any()) and not bool(mask.all())
    t = dx * mask
    assert int(t.abs().sum((0, 2, 3)).max()) < SUM_LIMIT and int((t * yv).abs().sum((0, 2, 3)).max()) < SUM_LIMIT
    return t.sum((0, 2, 3)), (t * yv).sum((0, 2, 3))


def switch_operands(device, cin, cout, shape):
    """integer_operands with the consumer of dx: its raw conv output yv in {-1, 0, 1}, integer scale in {1, 2} and shift in
    {-1, 0, 1}, and its exact sums (b1, b2)."""
    B, H, W = shape
    o = integer_operands(SWITCH_SEED, B, cin, cout, H, W, device=device)
    gen = torch.Generator().manual_seed(SWITCH_SEED + 1)
    o.yv = torch.randint(-1, 2, tuple(o.dx.shape), generator=gen, dtype=torch.int64).to(device)
    o.cscale = torch.randint(1, 3, (cin,), generator=gen, dtype=torch.int64).to(device)
    o.cshift = torch.randint(-1, 2, (cin,), generator=gen, dtype=torch.int64).to(device)
    o.b1, o.b2 = consumer_sums(o.dx, o.yv, o.cscale, o.cshift)
    return o
