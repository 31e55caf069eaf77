"""Host: tests/wgrad_ref.py (the reference the generic weight-gradient path and the transposed conv are judged by)
against torch.autograd in float64. Nothing here touches a kernel: this is what keeps the GPU tests' reference honest.

 * conv_transpose_k2s2 and its three gradients == F.conv_transpose2d under autograd (<= 1e-12 max-rel), and exactly in int64;
 * the pixel tables address what the header's formula says (checked by looking pixels up in a buffer of unique ids);
 * wgrad_slabs summed over the splits == the autograd weight gradient for the three ways the engine drives insar_wgrad:
   a transposed conv (dy taps move over a stride-2 dy table), a 3x3 conv (x taps move through offx) and a dilated 3x3 conv
   (per-tap tables with out-of-bounds taps); each split owns exactly its K steps;
 * fold / reduce / colsum against plain sums and permutes."""
import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_ref as R

F64 = torch.float64
TOL = 1e-12


def _max_rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _rnd(g, *s):
    return torch.randn(*s, generator=g, dtype=F64)


def _ints(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g, dtype=torch.int64)


@pytest.mark.parametrize("shape,cout", [((2, 5, 3, 4), 7), ((1, 3, 1, 1), 2), ((3, 4, 5, 2), 4)])
def test_conv_transpose_reference_is_autograd(shape, cout):
    g = torch.Generator().manual_seed(3 + cout)
    B, cin, h, w = shape
    x, wt, bias = _rnd(g, *shape).requires_grad_(), _rnd(g, cin, cout, 2, 2).requires_grad_(), _rnd(g, cout).requires_grad_()
    dout = _rnd(g, B, cout, 2 * h, 2 * w)
    ref = F.conv_transpose2d(x, wt, bias, stride=2)
    ref.backward(dout)
    out = R.conv_transpose_k2s2(x.detach(), wt.detach(), bias.detach())
    dx, dw, db = R.conv_transpose_k2s2_backward(x.detach(), wt.detach(), dout)
    assert _max_rel(out, ref.detach()) <= TOL
    assert _max_rel(dx, x.grad) <= TOL and _max_rel(dw, wt.grad) <= TOL and _max_rel(db, bias.grad) <= TOL
    assert _max_rel(R.conv_transpose_k2s2(x.detach(), wt.detach()), F.conv_transpose2d(x, wt, None, stride=2).detach()) <= TOL
    # the input gradient is the stride-2 convolution of dout with the same weights (the identity the GPU test uses)
    assert _max_rel(dx, F.conv2d(dout, wt.detach(), stride=2)) <= TOL
    # int64 operands: the same numbers exactly
    xi, wi, bi = _ints(g, -3, 3, *shape), _ints(g, -3, 3, cin, cout, 2, 2), _ints(g, -3, 3, cout)
    di = _ints(g, -3, 3, B, cout, 2 * h, 2 * w)
    oi = R.conv_transpose_k2s2(xi, wi, bi)
    assert oi.dtype == torch.int64 and torch.equal(oi.double(), R.conv_transpose_k2s2(xi.double(), wi.double(), bi.double()))
    for a, b in zip(R.conv_transpose_k2s2_backward(xi, wi, di), R.conv_transpose_k2s2_backward(xi.double(), wi.double(), di.double())):
        assert a.dtype == torch.int64 and torch.equal(a.double(), b)


@pytest.mark.parametrize("B,H,W,s,tail", [(2, 3, 4, 1, 0), (2, 3, 4, 2, 0), (1, 5, 7, 1, 10), (3, 5, 7, 2, 0)])
def test_pixel_table_addresses_the_strided_grid(B, H, W, s, tail):
    Hb, Wb = H * s, W * s
    mpad = R.round_up(B * H * W, 64)
    tab = R.pixel_table(B, H, W, s, Hb, Wb, tail, mpad)
    ids = torch.arange(B * Hb * Wb, dtype=torch.int64).reshape(B, 1, Hb, Wb) + 1       # 0 = halo
    buf = R.pad_nhwc(ids)[:, 0]
    want = ids[:, 0, ::s, ::s].reshape(-1)
    assert torch.equal(buf[tab[:B * H * W]], want)
    assert torch.equal(tab[B * H * W:], torch.full((mpad - B * H * W,), tail, dtype=torch.int64))
    # the header's formula at a hand-computed entry: (n, h, w) = (B-1, H-1, W-1)
    assert int(tab[B * H * W - 1]) == ((B - 1) * (Hb + 2) + (H - 1) * s + 1) * (Wb + 2) + (W - 1) * s + 1


@pytest.mark.parametrize("s,dil", [(1, 1), (1, 2), (1, 12), (2, 1)])
def test_pixel_table_taps_is_zero_padding(s, dil):
    """Gathering through the per-tap tables == reading a zero-padded map at (h*s + dy, w*s + dx): in-bounds taps see their
    pixel, taps on the halo or beyond see zero. Beyond the halo the ENTRY is 0; on the halo it is the halo pixel's index."""
    B, Hb, Wb = 2, 8, 8
    H, W = Hb // s, Wb // s
    taps = [(dil * (r - 1), dil * (c - 1)) for r in range(3) for c in range(3)]
    mpad = R.round_up(B * H * W, 64)
    tab = R.pixel_table_taps(B, H, W, s, Hb, Wb, taps, mpad)
    ids = torch.arange(B * Hb * Wb, dtype=torch.int64).reshape(B, 1, Hb, Wb) + 1
    buf = R.pad_nhwc(ids)[:, 0]
    big = F.pad(ids, (16, 16, 16, 16))[:, 0]
    for t, (dy, dx) in enumerate(taps):
        want = torch.stack([big[n, 16 + h * s + dy, 16 + w * s + dx] for n in range(B) for h in range(H) for w in range(W)])
        assert torch.equal(buf[tab[t, :B * H * W]], want), (dy, dx)
        assert int(tab[t, B * H * W:].abs().max()) == 0 if mpad > B * H * W else True
        for p, (n, h, w) in enumerate((n, h, w) for n in range(B) for h in range(H) for w in range(W)):
            hh, ww = h * s + dy, w * s + dx
            inside_padded = -1 <= hh <= Hb and -1 <= ww <= Wb
            assert (int(tab[t, p]) != 0) == (inside_padded and not (n == 0 and hh == -1 and ww == -1))
    if dil == 12:       # every off-centre tap is beyond the halo everywhere on an 8 x 8 map
        assert int(tab[[0, 1, 2, 3, 5, 6, 7, 8]].abs().max()) == 0


def _splits_partition(part, x_pad, dy_pad, tabx, tabdy, offx, offdy, stride):
    """Each split's slab == the slab of a one-split call over that split's K steps alone."""
    nsplit, mpad = part.shape[0], tabdy.numel()
    ksteps = mpad // 64
    sps = -(-ksteps // nsplit)
    for s in range(nsplit):
        k0, k1 = min(s * sps, ksteps), min((s + 1) * sps, ksteps)
        if k0 >= k1:
            assert float(part[s].abs().max()) == 0.0
            continue
        rows = slice(64 * k0, 64 * k1)
        tx = torch.cat([tabx[t * stride: t * stride + mpad][rows] for t in range(len(offx))]) if stride else tabx[rows]
        one = R.wgrad_slabs(x_pad, dy_pad, tx, tabdy[rows], offx, offdy, 1, 64 * (k1 - k0) if stride else 0)
        assert torch.equal(one[0], part[s])


@pytest.mark.parametrize("nsplit", [1, 2, 3, 5])
def test_slabs_sum_to_the_transposed_conv_weight_gradient(nsplit):
    g = torch.Generator().manual_seed(11)
    B, cin, cout, h, w = 3, 5, 4, 5, 7                 # 105 pixels -> Mpad 128: live tail entries
    x, dout = _rnd(g, B, cin, h, w), _rnd(g, B, cout, 2 * h, 2 * w)
    wt = _rnd(g, cin, cout, 2, 2).requires_grad_()
    F.conv_transpose2d(x, wt, None, stride=2).backward(dout)
    mpad = R.round_up(B * h * w, 64)
    tabx = R.pixel_table(B, h, w, 1, h, w, 0, mpad)
    tabdy = R.pixel_table(B, h, w, 2, 2 * h, 2 * w, 0, mpad)
    offdy = [a * (2 * w + 2) + b for a, b in R.TAPS2]
    part = R.wgrad_slabs(R.pad_nhwc(x), R.pad_nhwc(dout), tabx, tabdy, [0] * 4, offdy, nsplit)
    assert part.shape == (nsplit, 4, cout, cin)
    assert _max_rel(R.reduce(part, 1), wt.grad.reshape(cin, cout, 4)) <= TOL
    assert _max_rel(R.reduce(part, 1).reshape(cin, cout, 2, 2), R.conv_transpose_k2s2_backward(x, wt.detach(), dout)[1]) <= TOL
    _splits_partition(part, R.pad_nhwc(x), R.pad_nhwc(dout), tabx, tabdy, [0] * 4, offdy, 0)


@pytest.mark.parametrize("nsplit", [1, 2, 4])
def test_slabs_sum_to_the_3x3_conv_weight_gradient(nsplit):
    g = torch.Generator().manual_seed(12)
    B, cin, cout, H, W = 2, 3, 5, 6, 9                 # 108 pixels -> Mpad 128
    x, dy = _rnd(g, B, cin, H, W), _rnd(g, B, cout, H, W)
    wt = _rnd(g, cout, cin, 3, 3).requires_grad_()
    F.conv2d(x, wt, padding=1).backward(dy)
    mpad = R.round_up(B * H * W, 64)
    tabx = R.pixel_table(B, H, W, 1, H, W, W + 3, mpad)      # taps move on x: tail = the first interior pixel
    tabdy = R.pixel_table(B, H, W, 1, H, W, 0, mpad)         # tail = the zero halo corner
    offx = [(r - 1) * (W + 2) + (c - 1) for r in range(3) for c in range(3)]
    part = R.wgrad_slabs(R.pad_nhwc(x), R.pad_nhwc(dy), tabx, tabdy, offx, [0] * 9, nsplit)
    assert _max_rel(R.reduce(part, 0), wt.grad.reshape(cout, cin, 9)) <= TOL
    _splits_partition(part, R.pad_nhwc(x), R.pad_nhwc(dy), tabx, tabdy, offx, [0] * 9, 0)


@pytest.mark.parametrize("stride,dil,nsplit", [(1, 2, 1), (1, 2, 3), (1, 12, 2), (2, 1, 2)])
def test_slabs_sum_to_the_dilated_conv_weight_gradient_through_per_tap_tables(stride, dil, nsplit):
    g = torch.Generator().manual_seed(13)
    B, cin, cout, H, W = 2, 4, 3, 8, 8
    x = _rnd(g, B, cin, H, W)
    wt = _rnd(g, cout, cin, 3, 3).requires_grad_()
    y = F.conv2d(x, wt, stride=stride, padding=dil, dilation=dil)
    dy = _rnd(g, *y.shape)
    y.backward(dy)
    Ho, Wo = y.shape[2:]
    mpad = R.round_up(B * Ho * Wo, 64)
    taps = [(dil * (r - 1), dil * (c - 1)) for r in range(3) for c in range(3)]
    tabx = R.pixel_table_taps(B, Ho, Wo, stride, H, W, taps, mpad).reshape(-1)
    tabdy = R.pixel_table(B, Ho, Wo, 1, Ho, Wo, 0, mpad)
    part = R.wgrad_slabs(R.pad_nhwc(x), R.pad_nhwc(dy), tabx, tabdy, [0] * 9, [0] * 9, nsplit, tabx_tap_stride=mpad)
    assert _max_rel(R.reduce(part, 0), wt.grad.reshape(cout, cin, 9)) <= TOL
    _splits_partition(part, R.pad_nhwc(x), R.pad_nhwc(dy), tabx, tabdy, [0] * 9, [0] * 9, mpad)


def test_integer_slabs_are_exact():
    g = torch.Generator().manual_seed(14)
    B, cin, cout, h, w = 2, 4, 6, 8, 8
    x, dout = _ints(g, -3, 3, B, cin, h, w), _ints(g, -3, 3, B, cout, 2 * h, 2 * w)
    tabx = R.pixel_table(B, h, w, 1, h, w, 0, 128)
    tabdy = R.pixel_table(B, h, w, 2, 2 * h, 2 * w, 0, 128)
    offdy = [a * (2 * w + 2) + b for a, b in R.TAPS2]
    part = R.wgrad_slabs(R.pad_nhwc(x), R.pad_nhwc(dout), tabx, tabdy, [0] * 4, offdy, 2)
    assert part.dtype == torch.int64
    dw = R.conv_transpose_k2s2_backward(x, torch.zeros(cin, cout, 2, 2, dtype=torch.int64), dout)[1]
    assert torch.equal(R.reduce(part, 1).reshape(cin, cout, 2, 2), dw)


@pytest.mark.parametrize("nsplit,group", [(1, 8), (7, 8), (8, 8), (9, 8), (49, 8), (97, 16), (100, 16)])
def test_fold_and_reduce(nsplit, group):
    g = torch.Generator().manual_seed(nsplit)
    part = _ints(g, -1000, 1000, nsplit, 4, 3, 6)
    f = R.fold(part, group)
    assert f.shape[0] == -(-nsplit // group)
    for i in range(f.shape[0]):
        assert torch.equal(f[i], part[i * group:min((i + 1) * group, nsplit)].sum(0))
    total = part.sum(0)                                                   # [tap][co][ci]
    g0, g1 = R.reduce(part, 0), R.reduce(part, 1)
    assert g0.shape == (3, 6, 4) and g1.shape == (6, 3, 4)
    for tap in range(4):
        for co in range(3):
            for ci in range(6):
                assert int(g0.reshape(-1)[(co * 6 + ci) * 4 + tap]) == int(total[tap, co, ci])      # the header's layout 0
                assert int(g1.reshape(-1)[(ci * 3 + co) * 4 + tap]) == int(total[tap, co, ci])      # the header's layout 1
    assert torch.equal(R.reduce(f, 1), g1)
    base = _ints(g, -50, 50, 6, 3, 4)
    assert torch.equal(R.reduce(part, 1, accumulate_into=base), base + g1)


def test_colsum_reference():
    g = torch.Generator().manual_seed(5)
    part = _ints(g, -100, 100, 3 * 10 * 12)
    out = R.colsum(part, 3, 10, 5, ld=12)
    for s in range(3):
        for c in range(5):
            assert int(out[s, c]) == sum(int(part[(s * 10 + r) * 12 + c]) for r in range(10))
    assert torch.equal(R.colsum(part, 3, 10, 12), part.reshape(3, 10, 12).sum(1))
    base = _ints(g, -9, 9, 3, 5)
    assert torch.equal(R.colsum(part, 3, 10, 5, ld=12, accumulate_into=base), base + out)
    p = R.colsum_partial(part[:70], 10, 7, 4)
    assert p.shape == (3, 7) and torch.equal(p[2], part[:70].reshape(10, 7)[8:].sum(0)) and torch.equal(p.sum(0), part[:70].reshape(10, 7).sum(0))
