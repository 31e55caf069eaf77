"""CPU: tests/conv_ref.py (the int64 / float64 statement of the 3x3 convolution family that
tests/test_conv3x3_exact_gpu.py holds the kernels to) against torch.nn.functional in float64 and against autograd, the
operand recipe's exactness conditions, and the reason the exact GPU tests exist: three planted indexing errors of the kind
the hand-written staging code could make, each of which the exact comparison rejects, and what the criteria of
tests/test_parity_gpu.py (max_rel <= 6e-3 for bf16 outputs, 1e-4 for the statistics slab) make of the same error on that
file's own float operands. The figures in the docstrings below are computed by the tests themselves (and asserted)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import closed_form as cf
from tests import conv_ref as R
from tests.helpers import max_rel

OLD_OUT_TOL = 6e-3        # tests/test_parity_gpu.py: bf16 outputs, "only the output rounding remains"
OLD_STAT_TOL = 1e-4       # ... the statistics slab against sums of the stored output

CASES = [   # B, cin, cout, H, W, dil, stride
    (2, 8, 16, 7, 9, 1, 1), (1, 16, 8, 5, 5, 1, 2), (2, 8, 8, 8, 6, 1, 2), (2, 8, 16, 9, 8, 2, 1), (1, 8, 8, 12, 10, 3, 1),
    (1, 8, 8, 9, 11, 4, 1), (1, 8, 8, 1, 1, 1, 1), (1, 8, 8, 2, 3, 1, 2),
]


@pytest.mark.parametrize("B,cin,cout,H,W,dil,stride", CASES)
def test_reference_against_torch_float64(B, cin, cout, H, W, dil, stride):
    """Integer operands through the int64 path and the same values through the float64 path, forward and input gradient,
    against F.conv2d / F.conv_transpose2d in float64 (sums of a few hundred small integers: exact there too)."""
    o = R.integer_operands(3, B, cin, cout, H, W, dil, stride, q=1.0)
    xd, wd, gd = o.x.double(), o.w.double(), o.g.double()
    want_y = F.conv2d(xd, wd, padding=dil, dilation=dil, stride=stride)
    assert tuple(o.y.shape) == tuple(want_y.shape) and torch.equal(o.y.double(), want_y)
    assert torch.equal(R.conv3x3(xd, wd, dil, stride), want_y)
    opad = ((H - 1) % stride, (W - 1) % stride)               # the rows / columns of x beyond the last stride step
    want_dx = F.conv_transpose2d(gd, wd, padding=dil, dilation=dil, stride=stride, output_padding=opad)
    assert tuple(want_dx.shape) == (B, cin, H, W) and torch.equal(o.dx.double(), want_dx)
    assert torch.equal(R.conv3x3_input_grad(gd, wd, (H, W), dil, stride), want_dx)
    bias = torch.arange(cout, dtype=torch.int64) - 3
    assert torch.equal(R.conv3x3(o.x, o.w, dil, stride, bias).double(), F.conv2d(xd, wd, bias.double(), padding=dil, dilation=dil, stride=stride))
    s1, s2 = R.channel_stats(o.y)
    assert torch.equal(s1, o.s1) and torch.equal(s2, o.s2)
    assert torch.equal(s1.double(), want_y.sum((0, 2, 3))) and torch.equal(s2.double(), (want_y ** 2).sum((0, 2, 3)))


@pytest.mark.parametrize("B,cin,cout,H,W,dil,stride", CASES[:5])
def test_reference_input_gradient_against_autograd(B, cin, cout, H, W, dil, stride):
    """Non-integer float64 operands: dx is autograd's gradient of F.conv2d (to float64 rounding: the summation orders differ)."""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((B, cin, H, W), generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn((cout, cin, 3, 3), generator=gen, dtype=torch.float64)
    y = F.conv2d(x, w, padding=dil, dilation=dil, stride=stride)
    g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(g)
    assert max_rel(R.conv3x3(x.detach(), w, dil, stride), y.detach()) <= 1e-13
    assert max_rel(R.conv3x3_input_grad(g, w, (H, W), dil, stride), x.grad) <= 1e-13


def test_operand_recipe_is_seeded_and_sparse_where_channels_are_many():
    a = R.integer_operands(7, 1, 64, 256, 6, 6)
    b = R.integer_operands(7, 1, 64, 256, 6, 6)
    c = R.integer_operands(8, 1, 64, 256, 6, 6)
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("x", "w", "g", "y", "dx"))
    assert not torch.equal(a.x, c.x) and not torch.equal(a.w, c.w)
    for t in (a.x, a.w, a.g):
        assert int(t.min()) == -1 and int(t.max()) == 1
    assert R.weight_keep_probability(64, 256) == 1 / 16 and R.weight_keep_probability(8, 16) == 1.0
    dense = float((a.w != 0).double().mean())
    assert abs(dense - (2 / 3) / 16) < 0.01                  # kept with probability 1/16, non-zero two times in three
    assert float((a.y != 0).double().mean()) > 0.5           # ... and still most outputs are non-zero


def test_operand_recipe_refuses_operands_that_bf16_or_fp32_cannot_hold():
    """The conditions are asserted, not assumed: 257 needs nine significant bits, and 256 is the last value that does not."""
    R.assert_exact_in_bf16(torch.tensor([256, -256]))
    with pytest.raises(AssertionError):
        R.assert_exact_in_bf16(torch.tensor([3, -257]))
    with pytest.raises(AssertionError):
        R.integer_operands(1, 1, 8, 8, 4, 4, q=1.0, lo=-200, hi=200)   # sums of up to 72 products of size up to 200
    big = torch.full((1, 1, 300, 300), 16, dtype=torch.int64)        # 90000 * 256 >= 2^24
    R.assert_exact_in_bf16(big)
    with pytest.raises(AssertionError):
        R.assert_sums_exact_in_fp32(big)


# ---- three planted errors ---------------------------------------------------------------------------------------------------
def drop_one_product_in_the_last_column(x, w, y, ci=5, co=3):
    """The centre tap's product of input channel ci is missing from output channel co in the last image column (an edge-lane
    fragment cleared one element too wide)."""
    bad = y.clone()
    bad[:, co, :, -1] -= x[:, ci, :, -1] * w[co, ci, 1, 1]
    return bad


def first_pixel_reads_the_previous_image(x, w, y):
    """Output pixel (0, 0) of image 1 takes its centre tap from the last pixel of image 0 (a tile that straddles two images,
    staged one pixel too early)."""
    bad = y.clone()
    wc = w[:, :, 1, 1]
    bad[1, :, 0, 0] += (wc * (x[0, :, -1, -1] - x[1, :, 0, 0])[None, :]).sum(1)
    return bad


def stats_without_one_pixel(y, n=0, oy=0, ox=0):
    s1, s2 = R.channel_stats(y)
    return s1 - y[n, :, oy, ox], s2 - y[n, :, oy, ox] ** 2


def _old_fixture(cin, cout, shape):
    """The float operands of tests/test_parity_gpu.py's float64 tests, rounded to bf16 as the kernels see them."""
    x = cf.make_input(shape).bfloat16().double()
    w = cf.fill_tensor("weight", (cout, cin, 3, 3), 11).bfloat16().double()
    return x, w, R.conv3x3(x, w)


@pytest.fixture(scope="module")
def ints():
    return R.integer_operands(11, 3, 64, 64, 30, 30)


@pytest.fixture(scope="module")
def old_small():
    return _old_fixture(64, 64, (3, 64, 30, 30))          # test_conv3x3_flat_against_float64 / _c64_: tiles straddle images


@pytest.fixture(scope="module")
def old_deep():
    return _old_fixture(256, 128, (1, 256, 32, 32))       # test_conv3x3_flat_against_float64: four K slabs per tap


@pytest.fixture(scope="module")
def old_large():
    return _old_fixture(64, 64, (1, 64, 256, 256))        # 65,536 pixels per channel


def test_missing_product_in_the_last_column_is_rejected_exactly(ints, old_small, old_deep):
    """Exact comparison on the integer operands: rejected (59 of 172,800 outputs differ, each by 1).
    Old criterion (max_rel <= 6e-3) on the old operands: 64 -> 64 at 3 x 30 x 30 max_rel = 1.55e-2, rejected;
    256 -> 128 at 1 x 32 x 32 max_rel = 1.78e-3 — ACCEPTED. From 256 input channels on, the float64 tests cannot see an
    input channel that is missing from an output channel along a whole image edge."""
    bad = drop_one_product_in_the_last_column(ints.x, ints.w, ints.y, co=int(ints.w[:, 5, 1, 1].abs().argmax()))
    assert not torch.equal(bad, ints.y)
    print("integer operands: %d of %d outputs differ, by at most %d" % (int((bad != ints.y).sum()), ints.y.numel(), int((bad - ints.y).abs().max())))
    figs = [max_rel(drop_one_product_in_the_last_column(x, w, y), y) for x, w, y in (old_small, old_deep)]
    print("old criterion, dropped product: max_rel = %.3e (64 channels), %.3e (256 channels)" % tuple(figs))
    assert figs[0] > OLD_OUT_TOL
    assert 0 < figs[1] <= OLD_OUT_TOL


def test_pixel_read_from_the_previous_image_is_rejected_exactly(ints, old_small):
    """Exact comparison on the integer operands: rejected (the 64 outputs of that one pixel are at stake).
    Old criterion on the old operands (64 -> 64, 3 x 30 x 30): max_rel = 1.30e-1, rejected too: the closed-form images differ
    enough from one another that a whole pixel taken from the wrong image moves an output by an eighth of the largest."""
    bad = first_pixel_reads_the_previous_image(ints.x, ints.w, ints.y)
    assert not torch.equal(bad, ints.y)
    x, w, y = old_small
    fig = max_rel(first_pixel_reads_the_previous_image(x, w, y), y)
    print("old criterion, pixel from the previous image: max_rel = %.3e" % fig)
    assert fig > OLD_OUT_TOL


def test_pixel_left_out_of_the_statistics_is_rejected_exactly(ints, old_small, old_large):
    """Exact comparison on the integer operands: both sums differ, rejected.
    Old criterion (1e-4 of the largest per-channel sum, for the sums and for the sums of squares) on the old operands,
    pixel (0, 0) of image 0 dropped:
      64 -> 64, 3 x 30 x 30 (2,700 pixels): sum 2.99e-1, sum of squares 5.33e-4: both rejected;
      64 -> 64, 1 x 256 x 256 (65,536 pixels): sum 9.13e-3, rejected (the closed-form operands' per-channel sums nearly
      cancel, which makes that check sharp); sum of squares 3.30e-6 — ACCEPTED: the second column of the slab could lose
      a pixel unseen."""
    assert int(ints.y[0, :, 0, 0].abs().max()) > 0
    b1, b2 = stats_without_one_pixel(ints.y)
    assert not torch.equal(b1, ints.s1) and not torch.equal(b2, ints.s2)
    figs = []
    for x, w, y in (old_small, old_large):
        s1, s2 = R.channel_stats(y)
        b1, b2 = stats_without_one_pixel(y)
        figs.append((max_rel(b1, s1), max_rel(b2, s2)))
        print("old criterion, one pixel of %d dropped: sum %.3e, sum of squares %.3e" % ((y.numel() // y.shape[1],) + figs[-1]))
    assert min(figs[0]) > OLD_STAT_TOL
    assert figs[1][0] > OLD_STAT_TOL
    assert 0 < figs[1][1] <= OLD_STAT_TOL


@pytest.mark.parametrize("layer", R.SWITCH_ROUTE_LAYERS, ids=lambda l: f"{l[0]}-{l[1]}-" + "x".join(map(str, l[2])))
def test_switch_route_operands_are_exact_in_bf16_and_fp32(layer):
    """The operands of tests/test_switch_routes_gpu.py at each of its shapes: |y|, |dx| <= 256 (bf16 holds them), the
    per-channel sums of |y| and y^2 and the consumer's sums of |dx * mask| and |dx * mask * yv| below 2^24 (any fp32
    summation order is exact). The generator asserts these; here the margins are printed and held."""
    cin, cout, shape = layer
    o = R.switch_operands("cpu", cin, cout, shape)
    out = max(int(o.y.abs().max()), int(o.dx.abs().max()))
    sums = max(int(o.y.abs().sum((0, 2, 3)).max()), int((o.y * o.y).sum((0, 2, 3)).max()))
    mask = (o.cscale.reshape(1, -1, 1, 1) * o.yv + o.cshift.reshape(1, -1, 1, 1) > 0).to(torch.int64)
    cons = max(int((o.dx * mask).abs().sum((0, 2, 3)).max()), int((o.dx * mask * o.yv).abs().sum((0, 2, 3)).max()))
    print("%s: largest output %d (limit %d), largest per-channel sum %d, consumer sum %d (limit %d)" % (layer, out, R.OUT_LIMIT, sums, cons, R.SUM_LIMIT))
    assert out <= R.OUT_LIMIT and sums < R.SUM_LIMIT and cons < R.SUM_LIMIT
