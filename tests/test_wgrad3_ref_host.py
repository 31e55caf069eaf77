"""CPU: tests/wgrad3_ref.py (the int64 / float64 statement of the 3x3 weight gradient and of the row-of-taps kernels' split-K
slabs that tests/test_wgrad3_exact_gpu.py holds the kernels to) against torch.autograd on F.conv2d in float64; the address
probes decoded on the reference itself; and the reason the exact GPU tests exist: five planted staging / partition errors of
the kind the hand-written row-of-taps code could make, each rejected by the exact per-slab comparison, with what the present
criterion of tests/test_parity_gpu.py (max_rel of the FOLDED gradient <= 5 * KERNEL_TOL = 1e-4, on that file's closed-form
float operands rounded to bf16) makes of the same error at the same shape. The figures in the docstrings are computed by the
tests themselves, printed, and their side of the criterion asserted."""
import pytest
import torch
import torch.nn.functional as F

from oracle import closed_form as cf
from tests import conv_ref as R
from tests import wgrad3_ref as G
from tests.helpers import max_rel

OLD_TOL = 5 * 2e-5        # tests/test_parity_gpu.py: max_rel(gwt, wv.grad) <= KERNEL_TOL * 5

# every W regime: a K step inside an image row (W = 64, 128, 256), two and four image rows per step (W = 32, 16), one step
# per image, one step in all; the last two with wgrad3k's steps (KS * 32 pixels, KS slices)
GRIDS = [  # B, H, W, step_pixels, slices
    (2, 3, 64, 64, 1), (1, 2, 128, 64, 1), (2, 4, 32, 64, 1), (2, 8, 16, 64, 1), (3, 4, 16, 64, 1), (1, 1, 64, 64, 1),
    (2, 2, 256, 256, 8), (1, 3, 256, 128, 4), (1, 1, 64, 64, 2),
]


def _nsplits(ksteps):
    return sorted({1, 2, 3, max(1, ksteps // 2), ksteps, ksteps + 3, max(1, (ksteps + 4) // 5)})


def _autograd_dw(x, g):
    w = torch.zeros((g.shape[1], x.shape[1], 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, padding=1).backward(g.double())
    return w.grad


@pytest.mark.parametrize("B,H,W,step,slices", GRIDS)
def test_reference_against_autograd_and_slabs_sum_to_it(B, H, W, step, slices):
    """Integer operands: dw equals autograd's gradient of F.conv2d in float64 exactly (sums of a few hundred values in
    {-1, 0, 1}); for every nsplit the slabs sum to it, the splits beyond the last K step are zero, and a slab is what the
    reference gives for its own pixels alone. Float64 operands: the same to rounding."""
    o = G.integer_operands(5, B, 8, 16, H, W)
    assert torch.equal(o.dw.double(), _autograd_dw(o.x, o.g))
    ksteps = G.num_steps(B, H, W, step)
    for nsplit in _nsplits(ksteps):
        part = G.row_tap_slabs(o.x, o.g, nsplit, step, slices)
        assert tuple(part.shape) == (nsplit * slices, 9, 16, 8)
        assert torch.equal(G.fold(part), o.dw), nsplit
        sps = -(-ksteps // nsplit)
        for s in range(nsplit):
            if s * sps >= ksteps:
                assert not bool(part[s * slices:(s + 1) * slices].any()), (nsplit, s)
    # one slab on its own: split 1 of 2 (or the only one), last slice — only its pixels' products
    nsplit = min(2, ksteps)
    part = G.row_tap_slabs(o.x, o.g, nsplit, step, slices)
    sps = -(-ksteps // nsplit)
    s, sl = nsplit - 1, slices - 1
    keep = torch.zeros(B * H * W, dtype=torch.bool)
    for k in range(s * sps, min((s + 1) * sps, ksteps)):
        lo = k * step + (sl * G.SLICE if slices > 1 else 0)
        keep[lo:lo + (G.SLICE if slices > 1 else step)] = True
    g_only = o.g * keep.reshape(B, 1, H, W).to(torch.int64)
    assert torch.equal(part[s * slices + sl], G.row_tap_slabs(o.x, g_only, 1, step, 1)[0])
    gen = torch.Generator().manual_seed(3)
    xf = torch.randn((B, 8, H, W), generator=gen, dtype=torch.float64)
    gf = torch.randn((B, 16, H, W), generator=gen, dtype=torch.float64)
    assert max_rel(G.conv3x3_weight_grad(xf, gf), _autograd_dw(xf, gf)) <= 1e-13
    assert max_rel(G.fold(G.row_tap_slabs(xf, gf, 3, step, slices)), _autograd_dw(xf, gf)) <= 1e-13


def test_operand_recipe_bounds_every_partial_sum():
    o = G.integer_operands(7, 2, 64, 64, 3, 64)
    assert int(o.x.min()) == -1 and int(o.x.max()) == 1 and int(o.g.min()) == -1 and int(o.g.max()) == 1
    assert o.x.shape[0] * o.x.shape[2] * o.x.shape[3] < R.SUM_LIMIT
    with pytest.raises(AssertionError):
        G.integer_operands(7, 2 ** 12, 1, 1, 64, 64)                     # 2^24 pixels: a sum could leave fp32's integers
    with pytest.raises(AssertionError):
        big = torch.full((1, 1, 1, 64), 2 ** 27, dtype=torch.int64)
        G.conv3x3_weight_grad(big, big)                                  # 64 * 2^54: beyond float64's integers


@pytest.mark.parametrize("kind", ["x", "dy"])
@pytest.mark.parametrize("B,H,W,step,slices", GRIDS)
def test_probe_decoded_on_the_reference_names_the_right_pixels(kind, B, H, W, step, slices):
    """The probes on the reference's own slabs: every hot channel and tap decodes to the pixel one tap on (x probe) / one tap
    back (dy probe), 0 where that leaves the image; the hot pixels include both ends of every image, row and K step."""
    pr = G.probe_operands(kind, B, 64, 64, H, W, step, G.SLICE if slices > 1 else None)
    hot = set(pr.hot)
    assert len(pr.hot) == len(hot) <= 64
    for unit in (H * W, W, step):
        if 2 * (B * H * W // unit) <= 64:
            assert all(s in hot and s + unit - 1 in hot for s in range(0, B * H * W, unit)), unit
    nsplit = G.num_steps(B, H, W, step)
    part = G.row_tap_slabs(pr.x, pr.g, nsplit, step, slices)
    assert G.probe_report(pr, part) == ""
    got = G.decode_probe(kind, part)
    seen_halo = seen_pixel = 0
    for c, p in enumerate(pr.hot):
        n, r = divmod(p, H * W)
        h, w = r // W, r % W
        for tap, (ky, kx) in enumerate(G.TAPS):
            sgn = 1 if kind == "x" else -1
            hh, ww = h + sgn * (ky - 1), w + sgn * (kx - 1)
            if 0 <= hh < H and 0 <= ww < W:
                assert G.unpad_index(int(got[tap, c]), H, W) == (n, hh, ww)
                seen_pixel += 1
            else:
                assert int(got[tap, c]) == 0
                seen_halo += 1
    assert seen_halo and seen_pixel
    # a slab with one pixel taken from elsewhere is named: channel 0's centre tap moved one pixel on
    bad = part.clone()
    tapc = 4
    src = torch.zeros(64, dtype=torch.int64)
    wrong = G.expected_probe_index(pr, 0, tapc) + 1
    src[:G.CODE_BITS] = (wrong >> torch.arange(G.CODE_BITS)) & 1
    if kind == "x":
        bad[:, tapc, 0, :] = 0
        bad[0, tapc, 0, :] = src
    else:
        bad[:, tapc, :, 0] = 0
        bad[0, tapc, :, 0] = src
    report = G.probe_report(pr, bad)
    assert f"fetched padded pixel {wrong} " in report and f"expected padded pixel {wrong - 1} " in report, report


# ---- five planted errors -----------------------------------------------------------------------------------------------------
def _slab_of(p, ksteps, nsplit, step, slices):
    k = p // step
    return G.split_of_step(k, ksteps, nsplit) * slices + ((p % step) // G.SLICE if slices > 1 else 0)


def refetch(part, x, g, nsplit, step, slices, fixes):
    """A copy of `part` in which, for every (p, tap, shift) of `fixes`, pixel p's products under `tap` take x from the padded
    pixel `shift` positions away from the right one (None: from nowhere, the products are dropped)."""
    B, ci, H, W = x.shape
    xp = torch.zeros((B, H + 2, W + 2, ci), dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    xp = xp.reshape(-1, ci)
    g_rows = g.permute(0, 2, 3, 1).reshape(B * H * W, -1)
    ksteps = G.num_steps(B, H, W, step)
    bad = part.clone()
    for p, tap, shift in fixes:
        n, r = divmod(p, H * W)
        ky, kx = G.TAPS[tap]
        right = G.padded_index(n, r // W + ky - 1, r % W + kx - 1, H, W)
        wrong = torch.zeros_like(xp[0]) if shift is None else xp[max(right + shift, 0)]
        bad[_slab_of(p, ksteps, nsplit, step, slices), tap] += torch.outer(g_rows[p], wrong - xp[right])
    return bad


def lead_pixel_from_the_previous_row(B, H, W):
    """kx = 0 of the first pixel of every image row reads two padded pixels early: the last pixel of the row above (the X run
    staged without its halo pixels)."""
    return [(p, 3 * ky, -2) for p in range(0, B * H * W, W) for ky in range(3)]


def tail_pixel_of_a_step_dropped(B, H, W, step=G.STEP):
    """kx = 2 of the last pixel of every K step finds nothing (the X run staged with a lead but without a tail)."""
    return [(p, 3 * ky + 2, None) for p in range(step - 1, B * H * W, step) for ky in range(3)]


def second_row_of_a_step_offset_by_w(B, H, W, step=G.STEP):
    """W = 16: the second image row of every K step is read W pixels after the first instead of W + 2: all nine taps of its
    pixels land two padded pixels early."""
    rows_per_step = step // W
    return [(p, tap, -2) for p in range(B * H * W) if (p // W) % rows_per_step == 1 for tap in range(9)]


def step_given_to_the_neighbouring_split(part, x, g, nsplit, step=G.STEP):
    """The first K step of split 1 is summed into split 0 (steps_per_split rounded the other way for one work-group)."""
    ksteps = G.num_steps(x.shape[0], x.shape[2], x.shape[3], step)
    sps = -(-ksteps // nsplit)
    one = G.row_tap_slabs(x, g, ksteps, step)[sps]
    bad = part.clone()
    bad[1] -= one
    bad[0] += one
    return bad


def slices_swapped(part, a=1, b=2):
    """Two of wgrad3k's slices of split 0 written to each other's slab."""
    bad = part.clone()
    bad[[a, b]] = part[[b, a]]
    return bad


def _float_operands(B, cin, cout, H, W):
    """tests/test_parity_gpu.py's operands of the weight-gradient checks, rounded to bf16 as the kernels see them."""
    return cf.make_input((B, cin, H, W)).bfloat16().double(), cf.make_grad((B, cout, H, W)).bfloat16().double()


def _both(B, H, W, nsplit, step, slices, plant, seed=11, cin=64, cout=64):
    """(exact comparison rejects?, slabs that differ, max_rel of the folded gradient on the float operands)."""
    o = G.integer_operands(seed, B, cin, cout, H, W)
    part = G.row_tap_slabs(o.x, o.g, nsplit, step, slices)
    bad = plant(part, o.x, o.g)
    differ = int((bad != part).flatten(1).any(1).sum())
    xf, gf = _float_operands(B, cin, cout, H, W)
    partf = G.row_tap_slabs(xf, gf, nsplit, step, slices)
    fig = max_rel(G.fold(plant(partf, xf, gf)), G.fold(partf))
    return not torch.equal(bad, part), differ, fig


def test_lead_pixel_from_the_previous_row_is_rejected_exactly():
    """64 -> 64 at (2, 3, 64), nsplit = 3. Exact comparison: rejected (all three slabs differ).
    Present criterion on the float operands: max_rel = 4.53e-1, rejected too — the closed-form gradient is a wave whose
    products largely cancel in the sum over pixels, so the folded gradient is small beside a single row's stray products."""
    B, H, W, nsplit = 2, 3, 64, 3
    fixes = lead_pixel_from_the_previous_row(B, H, W)
    rejected, differ, fig = _both(B, H, W, nsplit, 64, 1, lambda part, x, g: refetch(part, x, g, nsplit, 64, 1, fixes))
    print("lead pixel from the previous row: %d of %d slabs differ; present criterion max_rel = %.3e" % (differ, nsplit, fig))
    assert rejected and differ == nsplit
    assert fig > OLD_TOL


def test_dropped_tail_pixel_of_a_step_is_rejected_exactly():
    """64 -> 64 at (1, 2, 128) (two K steps per image row: the first one's tail is a real pixel), nsplit = 2. Exact
    comparison: rejected. Present criterion: max_rel = 4.60e-1, rejected too."""
    B, H, W, nsplit = 1, 2, 128, 2
    fixes = tail_pixel_of_a_step_dropped(B, H, W)
    rejected, differ, fig = _both(B, H, W, nsplit, 64, 1, lambda part, x, g: refetch(part, x, g, nsplit, 64, 1, fixes))
    print("tail pixel of a K step dropped: %d of %d slabs differ; present criterion max_rel = %.3e" % (differ, nsplit, fig))
    assert rejected and differ == nsplit
    assert fig > OLD_TOL


def test_second_row_offset_by_w_is_rejected_exactly():
    """64 -> 64 at (2, 8, 16), nsplit = 4 (one K step of four image rows each). Exact comparison: rejected. Present
    criterion: max_rel = 8.19e-1, rejected too (a quarter of all products take a pixel two columns away)."""
    B, H, W, nsplit = 2, 8, 16, 4
    fixes = second_row_of_a_step_offset_by_w(B, H, W)
    rejected, differ, fig = _both(B, H, W, nsplit, 64, 1, lambda part, x, g: refetch(part, x, g, nsplit, 64, 1, fixes))
    print("second row of a step offset by W: %d of %d slabs differ; present criterion max_rel = %.3e" % (differ, nsplit, fig))
    assert rejected and differ == nsplit
    assert fig > OLD_TOL


def test_step_in_the_neighbouring_split_is_rejected_exactly():
    """64 -> 64 at (2, 3, 64), nsplit = 3. Exact per-slab comparison: rejected (slabs 0 and 1 differ). Present criterion:
    max_rel = 0 up to float64 rounding — ACCEPTED, by construction: the fold adds every slab, so which slab a K step's
    products land in cannot show in the folded gradient. Only a per-slab reference sees the partition."""
    B, H, W, nsplit = 2, 3, 64, 3
    rejected, differ, fig = _both(B, H, W, nsplit, 64, 1, lambda part, x, g: step_given_to_the_neighbouring_split(part, x, g, nsplit))
    print("K step in the neighbouring split: %d of %d slabs differ; present criterion max_rel = %.3e" % (differ, nsplit, fig))
    assert rejected and differ == 2
    assert fig <= 1e-13 < OLD_TOL


def test_swapped_slices_are_rejected_exactly():
    """wgrad3k's 64 -> 64 at (2, 2, 256) (K step = 256 pixels = 8 slices), nsplit = 2: 16 slabs. Exact per-slab comparison:
    rejected (slabs 1 and 2 differ). Present criterion: max_rel = 0 up to float64 rounding — ACCEPTED, by construction, as
    above: the slab order split * KS + slice is invisible after the fold."""
    B, H, W, nsplit = 2, 2, 256, 2
    rejected, differ, fig = _both(B, H, W, nsplit, 256, 8, lambda part, x, g: slices_swapped(part))
    print("two slices swapped: %d of %d slabs differ; present criterion max_rel = %.3e" % (differ, nsplit * 8, fig))
    assert rejected and differ == 2
    assert fig <= 1e-13 < OLD_TOL


def _lid(l):
    return f"{l[0]}-{l[1]}-" + "x".join(map(str, l[2]))


@pytest.mark.parametrize("layer", G.SWITCH_LAYERS, ids=_lid)
def test_switch_wgrad_operands_keep_every_partial_sum_exact(layer):
    """The layers of tests/test_switch_wgrad_gpu.py with its seed: |x|, |g| <= 1 and B*H*W < 2^24, so every partial sum of
    the products over ANY subset of the pixels (whatever nsplit and slab partition the engine picks) is an integer below
    2^24 in magnitude, which fp32 holds; the largest element of the reference gradient is printed and held to the bound."""
    cin, cout, (B, H, W) = layer
    o = G.integer_operands(G.SWITCH_SEED, B, cin, cout, H, W)
    big = int(o.dw.abs().max())
    print("%s: largest |dw| %d, pixels %d (limit %d)" % (layer, big, B * H * W, R.SUM_LIMIT))
    assert int(o.x.abs().max()) <= 1 and int(o.g.abs().max()) <= 1 and B * H * W < R.SUM_LIMIT and 0 < big < R.SUM_LIMIT


@pytest.mark.parametrize("layer", G.UNIT_LAYERS, ids=_lid)
def test_switch_unit_operands_and_reference(layer):
    """The 1x1 and the dilated unit of the WGRAD_FILL_DL cases: the same bound, and conv_weight_grad against autograd of
    torch.nn.functional.conv2d in float64 on a small grid of the same kind."""
    cin, cout, (B, H, W), k, dil = layer
    o = G.unit_operands(G.SWITCH_SEED, layer)
    big = int(o.dw.abs().max())
    print("%s: largest |dw| %d, pixels %d (limit %d)" % (layer, big, B * H * W, R.SUM_LIMIT))
    assert int(o.x.abs().max()) <= 1 and int(o.g.abs().max()) <= 1 and B * H * W < R.SUM_LIMIT and 0 < big < R.SUM_LIMIT
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((2, 5, 7, 9), generator=gen, dtype=torch.float64)
    g = torch.randn((2, 4, 7, 9), generator=gen, dtype=torch.float64)
    w = torch.zeros((4, 5, k, k), dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, padding=dil * (k // 2), dilation=dil).backward(g)
    assert max_rel(G.conv_weight_grad(x, g, k, dil), w.grad) <= 1e-13


def test_switch_transposed_conv_operands_keep_every_partial_sum_exact():
    """UpPlan's operands in the WGRAD_FILL_T cases (x in [-2, 2], dout in [-3, 3], one product per input pixel and tap for dW,
    four output pixels per input pixel for dbias): every partial sum below 2^24."""
    B, cin, h, w = G.UP_SHAPE
    assert G.UP_X_MAX * G.UP_G_MAX * B * h * w < R.SUM_LIMIT and G.UP_G_MAX * 4 * B * h * w < R.SUM_LIMIT
