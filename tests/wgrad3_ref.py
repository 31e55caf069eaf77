"""Reference statement of the 3x3 / stride-1 / pad-1 weight gradient and of the split-K slabs the four row-of-taps kernels
(insar_wgrad_conv3, _conv3x, _conv3y, _conv3k) write, from include/insar_hip.h and the formula at the top of
csrc/wgrad3.hip — not from kernel code — in plain torch int64 / float64, on its operands' device; the integer operand recipe
of tests/conv_ref.py under which every route has ONE right answer; and address probes whose slabs spell out which pixel a
kernel fetched. tests/test_wgrad3_ref_host.py holds it to torch.autograd; tests/test_wgrad3_exact_gpu.py holds the kernels
to it.

The operation. x [B][Ci][H][W], g [B][Co][H][W] (the upstream gradient, `dy` of the header):
    dw[co, ci, ky, kx] = sum_{n, oy, ox} g[n, co, oy, ox] * x[n, ci, oy + ky - 1, ox + kx - 1]          (zero outside x)

The slabs. Pixels are flattened p = (n*H + h)*W + w. A K step is `step_pixels` consecutive p (64 for conv3 / 3x / 3y, KS * 32
for 3k), ksteps = B*H*W / step_pixels; split s owns the steps [s*ceil(ksteps/nsplit), (s+1)*ceil(ksteps/nsplit)) clipped to
ksteps; slice sl (of `slices` = KS; 1 for the others) of a step owns the step's pixels [sl*32, sl*32 + 32) (all of them when
slices == 1):
    part[split*slices + sl][3*ky + kx][co][ci] = sum over the pixels of (split, sl) of g[p, co] * x[p + tap, ci]
A split without a step is all zeros.

Exactness. Every function takes int64 or float64 tensors. int64 operands are contracted in float64 — exact while every
partial sum stays below 2^53, which is asserted — and returned as int64.

Probes. A "padded pixel index" is the row of the padded NHWC buffer [B][H+2][W+2][C] flattened over pixels:
(n*(H+2) + h + 1)*(W+2) + w + 1 for the interior pixel (n, h, w); it is >= W + 3 there, so 0 can stand for "nothing".
 * x probe: x[p, ci] = bit ci of p's padded pixel index (ci < 24, zero beyond), g one-hot: output channel co is 1 at its hot
   pixel and nowhere else. Then sum_slabs part[tap][co][0:24] spells the index of the x pixel fetched for (hot pixel of co,
   tap) — 0 where the tap lands on the halo.
 * dy probe, the mirror image: x one-hot per input channel, g carries the code over co < 24; sum_slabs part[tap][0:24][ci]
   spells the index of the dy pixel that met ci's hot x pixel under that tap — the pixel one tap BACK from it, 0 where that
   is not a pixel of the image.
Hot pixels sit at the first and last pixel of every image, image row, K step and 32-pixel slice, and at the pixel on either
side of each (hot_pixels)."""
from types import SimpleNamespace

import torch

from tests import conv_ref as R

STEP = 64                # pixels per K step of insar_wgrad_conv3 / 3x / 3y
SLICE = 32               # pixels per slice of a step of insar_wgrad_conv3k (its K step: KS * 32)
CODE_BITS = 24           # channels that carry the bit code of a probe
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def _pixels_by_tap(x):
    """x [B][Ci][H][W] -> [9][B*H*W][Ci]: row p of tap (ky, kx) is x at p's pixel moved by (ky-1, kx-1), zero outside x."""
    B, ci, H, W = x.shape
    xp = torch.zeros((B, H + 2, W + 2, ci), dtype=x.dtype, device=x.device)
    xp[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    return torch.stack([xp[:, ky:ky + H, kx:kx + W].reshape(B * H * W, ci) for ky, kx in TAPS])


def _contract_units(g_rows, x_taps, unit):
    """g_rows [P][Co], x_taps [9][P][Ci] -> [P/unit][9][Co][Ci]: the sums over each run of `unit` consecutive pixels. int64
    operands exactly (through float64, bounded below 2^53)."""
    P, co = g_rows.shape
    ci = x_taps.shape[2]
    assert P % unit == 0
    exact = g_rows.dtype == torch.int64
    if exact:
        assert x_taps.dtype == torch.int64
        bound = float(g_rows.abs().max()) * float(x_taps.abs().max()) * P if P else 0.0
        assert bound < 2.0 ** 53
    else:
        assert g_rows.dtype == torch.float64 and x_taps.dtype == torch.float64
    gu = g_rows.double().reshape(P // unit, 1, unit, co).transpose(2, 3)                    # [U][1][Co][unit]
    xu = x_taps.double().reshape(9, P // unit, unit, ci).transpose(0, 1)                    # [U][9][unit][Ci]
    out = gu @ xu                                                                           # [U][9][Co][Ci]
    return out.to(torch.int64) if exact else out


def conv3x3_weight_grad(x, g):
    """dw of the module docstring: x [B][Ci][H][W], g [B][Co][H][W] -> [Co][Ci][3][3]."""
    B, ci, H, W = x.shape
    assert g.shape[0] == B and tuple(g.shape[2:]) == (H, W)
    co = g.shape[1]
    g_rows = g.permute(0, 2, 3, 1).reshape(B * H * W, co)
    dw = _contract_units(g_rows, _pixels_by_tap(x), B * H * W)[0]                           # [9][Co][Ci]
    return dw.permute(1, 2, 0).reshape(co, ci, 3, 3).contiguous()


def conv_weight_grad(x, g, k=3, dil=1):
    """dw of a k x k (k in {1, 3}) / stride-1 convolution with dilation dil and padding dil*(k-1)/2 (the 1x1 and dilated units of
    DeepLabV3-CA): dw[co, ci, ky, kx] = sum_{n, oy, ox} g[n, co, oy, ox] * x[n, ci, oy + (ky - k//2)*dil, ox + (kx - k//2)*dil],
    zero outside x. x [B][Ci][H][W], g [B][Co][H][W] -> [Co][Ci][k][k]; int64 exactly (through float64, bounded below 2^53)."""
    assert k in (1, 3) and dil >= 1
    B, ci, H, W = x.shape
    co = g.shape[1]
    assert g.shape[0] == B and tuple(g.shape[2:]) == (H, W)
    exact = x.dtype == torch.int64
    if exact:
        assert g.dtype == torch.int64 and float(x.abs().max()) * float(g.abs().max()) * B * H * W < 2.0 ** 53
    p = dil * (k // 2)
    xp = torch.zeros((B, H + 2 * p, W + 2 * p, ci), dtype=torch.float64, device=x.device)
    xp[:, p:p + H, p:p + W] = x.permute(0, 2, 3, 1).double()
    g_rows = g.permute(0, 2, 3, 1).reshape(B * H * W, co).double()
    dw = torch.zeros((co, ci, k, k), dtype=torch.float64, device=x.device)
    for ky in range(k):
        for kx in range(k):
            v = xp[:, ky * dil:ky * dil + H, kx * dil:kx * dil + W].reshape(B * H * W, ci)
            dw[:, :, ky, kx] = g_rows.t() @ v
    return dw.to(torch.int64) if exact else dw


def num_steps(B, H, W, step_pixels=STEP):
    assert (B * H * W) % step_pixels == 0
    return B * H * W // step_pixels


def split_of_step(k, ksteps, nsplit):
    """The split that owns K step k."""
    return k // -(-ksteps // nsplit)


def row_tap_slabs(x, g, nsplit, step_pixels=STEP, slices=1):
    """part of the module docstring: [nsplit * slices][9][Co][Ci]."""
    B, ci, H, W = x.shape
    co = g.shape[1]
    P = B * H * W
    assert nsplit >= 1 and slices >= 1 and step_pixels % slices == 0 and P % step_pixels == 0
    assert slices == 1 or step_pixels == slices * SLICE
    ksteps = P // step_pixels
    g_rows = g.permute(0, 2, 3, 1).reshape(P, co)
    units = _contract_units(g_rows, _pixels_by_tap(x), step_pixels // slices)               # [ksteps * slices][9][Co][Ci]
    units = units.reshape(ksteps, slices, 9, co, ci)
    sps = -(-ksteps // nsplit)
    part = torch.zeros((nsplit, slices, 9, co, ci), dtype=units.dtype, device=x.device)
    for s in range(nsplit):
        k0, k1 = min(s * sps, ksteps), min((s + 1) * sps, ksteps)
        if k0 < k1:
            part[s] = units[k0:k1].sum(0)
    return part.reshape(nsplit * slices, 9, co, ci)


def fold(part):
    """sum of the slabs, re-laid out as the torch parameter: [Co][Ci][3][3] (what insar_wgrad_reduce, layout 0, produces)."""
    t = part.sum(0)
    return t.permute(1, 2, 0).reshape(t.shape[1], t.shape[2], 3, 3).contiguous()


def integer_operands(seed, B, cin, cout, H, W, device="cpu"):
    """conv_ref.integer_operands' x and g (uniform in {-1, 0, 1}, the same values on every device) with dw =
    conv3x3_weight_grad(x, g). B*H*W < SUM_LIMIT is asserted: then every partial sum of the products, in ANY partition of the
    pixels, is an integer below 2^24 in magnitude and an fp32 accumulator holds it exactly."""
    assert B * H * W < R.SUM_LIMIT
    o = R.integer_operands(seed, B, cin, cout, H, W, device=device)
    assert int(o.x.abs().max()) <= 1 and int(o.g.abs().max()) <= 1
    return SimpleNamespace(x=o.x, g=o.g, dw=conv3x3_weight_grad(o.x, o.g))


# ---- the layers of tests/test_switch_wgrad_gpu.py (tests/test_wgrad3_ref_host.py asserts the exactness bound of each) -----------
SWITCH_SEED = 77
LAYER_128 = (128, 128, (4, 64, 64))        # wgrad3<128, 128>; 3y with WGRAD_Y & 2; 3k with WGRAD_K
LAYER_X = (256, 128, (4, 64, 64))          # wgrad3x<256, 128>; 3y with WGRAD_Y & 1; wgrad3 with WGRAD_X = 0
LAYER_DEEP = (512, 512, (2, 64, 64))       # 48 tiles of 128 x 128: the default grid cap binds
LAYER_ODD = (256, 256, (2, 8, 24))         # W = 24: no row-of-taps kernel, the per-tap kernel's 256 x 256 tile
SWITCH_LAYERS = [LAYER_128, LAYER_X, LAYER_DEEP, LAYER_ODD]
# (Cin, Cout, (B, H, W), k, dilation): the DeepLabV3-CA units of the WGRAD_FILL_DL cases
UNIT_1X1 = (512, 256, (2, 64, 64), 1, 1)
UNIT_DILATED = (128, 128, (2, 64, 64), 3, 2)
UNIT_LAYERS = [UNIT_1X1, UNIT_DILATED]
UP_SHAPE, UP_COUT = (4, 256, 32, 32), 256   # the transposed convolution of the WGRAD_FILL_T cases: x in [-2, 2], dout in [-3, 3]
UP_X_MAX, UP_G_MAX = 2, 3


def unit_operands(seed, layer, device="cpu"):
    """x, g uniform in {-1, 0, 1} (drawn on the CPU generator) and dw = conv_weight_grad of a UNIT_* layer."""
    cin, cout, (B, H, W), k, dil = layer
    assert B * H * W < R.SUM_LIMIT
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (B, cin, H, W), generator=gen, dtype=torch.int64).to(device)
    g = torch.randint(-1, 2, (B, cout, H, W), generator=gen, dtype=torch.int64).to(device)
    return SimpleNamespace(x=x, g=g, dw=conv_weight_grad(x, g, k, dil))


# ---- address probes ---------------------------------------------------------------------------------------------------------
def padded_index(n, h, w, H, W):
    return (n * (H + 2) + h + 1) * (W + 2) + w + 1


def unpad_index(idx, H, W):
    """(n, h, w) of a padded pixel index, h in -1 .. H and w in -1 .. W (the halo included)."""
    row, col = divmod(int(idx), W + 2)
    n, hp = divmod(row, H + 2)
    return n, hp - 1, col - 1


def hot_pixels(B, H, W, count, step_pixels=STEP, slice_pixels=None):
    """Up to `count` flattened pixels p, in ascending order: the first and last pixel of every image, image row and K step
    (and slice, when slice_pixels is given), then — while there is room — the pixel on either side of each. When they do not
    all fit, a class is thinned evenly (its first and last member kept), the interior ones first."""
    P = B * H * W
    edges = set()
    for unit in (H * W, W, step_pixels):
        for s in range(0, P, unit):
            edges.update((s, min(s + unit, P) - 1))
    slice_edges = set()
    if slice_pixels:
        for s in range(0, P, slice_pixels):
            slice_edges.update((s, s + slice_pixels - 1))
    slice_edges -= edges
    beside = {q for p in edges | slice_edges for q in (p - 1, p + 1) if 0 <= q < P} - edges - slice_edges
    chosen = []
    for cls in (sorted(edges), sorted(slice_edges), sorted(beside)):
        room = count - len(chosen)
        if room <= 0 or not cls:
            continue
        if len(cls) > room:
            cls = [cls[0]] if room == 1 else [cls[(i * (len(cls) - 1)) // (room - 1)] for i in range(room)]
        chosen += cls
    return sorted(set(chosen))


def code_image(B, H, W, channels, device="cpu", first_bit=0, bits=CODE_BITS):
    """[B][channels][H][W] int64: channel c < bits of pixel (n, h, w) holds bit first_bit + c of its padded pixel index."""
    n = torch.arange(B, device=device).reshape(B, 1, 1)
    h = torch.arange(H, device=device).reshape(1, H, 1)
    w = torch.arange(W, device=device).reshape(1, 1, W)
    idx = (n * (H + 2) + h + 1) * (W + 2) + w + 1
    assert int(idx.max()) < 2 ** CODE_BITS and channels >= bits
    img = torch.zeros((B, channels, H, W), dtype=torch.int64, device=device)
    for c in range(bits):
        img[:, c] = (idx >> (first_bit + c)) & 1
    return img


def one_hot_image(B, H, W, channels, hot, device="cpu"):
    """[B][channels][H][W] int64: channel c is 1 at the flattened pixel hot[c] and 0 elsewhere (all zero for c >= len(hot))."""
    img = torch.zeros((B, channels, H, W), dtype=torch.int64, device=device)
    for c, p in enumerate(hot):
        n, r = divmod(p, H * W)
        img[n, c, r // W, r % W] = 1
    return img


def probe_operands(kind, B, cin, cout, H, W, step_pixels=STEP, slice_pixels=None, device="cpu"):
    """kind "x": x carries the code, g is one-hot per output channel; kind "dy": x is one-hot per input channel, g carries the
    code. Returns x, g (int64, values 0 / 1) and hot: hot[c] = flattened pixel of one-hot channel c (channels beyond
    len(hot) are all zero)."""
    assert kind in ("x", "dy")
    hot = hot_pixels(B, H, W, cout if kind == "x" else cin, step_pixels, slice_pixels)
    if kind == "x":
        x, g = code_image(B, H, W, cin, device), one_hot_image(B, H, W, cout, hot, device)
    else:
        x, g = one_hot_image(B, H, W, cin, hot, device), code_image(B, H, W, cout, device)
    return SimpleNamespace(kind=kind, x=x, g=g, hot=hot, B=B, H=H, W=W)


def decode_probe(kind, part):
    """The pixel indices a probe's slabs spell: int64 [9][channels] (channels = Co for the x probe, Ci for the dy probe), -1
    where the code channels of the summed slabs hold anything but 0 / 1 (not one pixel: several, or garbage)."""
    t = part.double().sum(0)                                                # [9][Co][Ci]
    bits = t[:, :, :CODE_BITS] if kind == "x" else t[:, :CODE_BITS, :].transpose(1, 2)       # [9][channels][24]
    valid = ((bits == 0) | (bits == 1)).all(2)
    weights = (2 ** torch.arange(CODE_BITS, device=part.device)).double()
    idx = (torch.nan_to_num(bits) * weights).sum(2).to(torch.int64)
    return torch.where(valid, idx, torch.full_like(idx, -1))


def expected_probe_index(pr, c, tap):
    """The index decode_probe must give for one-hot channel c and tap: the x pixel one tap ON from the hot pixel (x probe) or
    the dy pixel one tap BACK (dy probe); 0 when that lies outside the image."""
    ky, kx = TAPS[tap]
    n, r = divmod(pr.hot[c], pr.H * pr.W)
    h, w = r // pr.W, r % pr.W
    sign = 1 if pr.kind == "x" else -1
    hh, ww = h + sign * (ky - 1), w + sign * (kx - 1)
    return padded_index(n, hh, ww, pr.H, pr.W) if 0 <= hh < pr.H and 0 <= ww < pr.W else 0


def _name(idx, H, W):
    if idx < 0:
        return "no single pixel (code channels hold values other than 0 / 1)"
    if idx == 0:
        return "nothing (zeros)"
    n, h, w = unpad_index(idx, H, W)
    where = "" if 0 <= h < H and 0 <= w < W else " [halo]"
    return f"padded pixel {idx} = (n {n}, h {h}, w {w}){where}"


def probe_report(pr, part, limit=6):
    """'' when the slabs spell the expected pixel for every hot channel and tap, else the first few that do not: which pixel
    the kernel fetched and which it should have."""
    got = decode_probe(pr.kind, part).cpu()
    lines = []
    for c, p in enumerate(pr.hot):
        for tap in range(9):
            want = expected_probe_index(pr, c, tap)
            if int(got[tap, c]) != want:
                n, r = divmod(p, pr.H * pr.W)
                lines.append(f"{pr.kind} probe, channel {c} hot at p = {p} (n {n}, h {r // pr.W}, w {r % pr.W}), tap (ky {TAPS[tap][0]}, kx {TAPS[tap][1]}): "
                             f"fetched {_name(int(got[tap, c]), pr.H, pr.W)}, expected {_name(want, pr.H, pr.W)}")
    more = f"; ... {len(lines) - limit} more" if len(lines) > limit else ""
    return "; ".join(lines[:limit]) + more
