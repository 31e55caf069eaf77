"""The case tables shared by tests/test_pointwise_ref_host.py (reference against torch, float32 floor, sensitivity) and the
GPU tests that hold the kernels to tests/pointwise_ref.py. CPU only: seeded inputs as STORED tensors. The reasons for the
shapes stand in the tables at the top of tests/test_forward_apply_gpu.py and tests/test_trunk_pointwise_gpu.py."""
import torch

from tests.test_bn_backward_chain_gpu import enforce_margin, make_case

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = {"fp32": F32, "bf16": BF16}


def tname(T):
    return "bf16" if T == BF16 else "fp32"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def gates(B, Cn, seed, lattice=False):
    """One gate row per image, all different, in (0.1, 1) — and one NEGATIVE value in the last image (a ReLU applied after the
    gate, or a gate taken from the neighbouring image, then shows)."""
    g = gen(seed)
    gt = torch.exp2(-torch.randint(0, 4, (B, Cn), generator=g).float()) if lattice else 0.1 + 0.9 * torch.rand(B, Cn, generator=g)
    gt[B - 1, 5 % Cn] = -0.75
    gt[0, 5 % Cn] = 0.5
    return gt


# ---------------------------------------------------------------------------------------------- BatchNorm apply family
# id -> (B, H, W, C, gate, relu)
APPLY_SHAPES = {
    "w1": (2, 3, 1, 64, 1, 1), "w15": (2, 2, 15, 64, 0, 1), "w16": (2, 3, 16, 64, 1, 0), "w17": (1, 3, 17, 64, 0, 0),
    "w31": (2, 2, 31, 64, 1, 1), "w32": (1, 2, 32, 64, 0, 1), "w33": (2, 2, 33, 64, 1, 0), "w65": (2, 2, 65, 64, 1, 1),
    "w129": (1, 2, 129, 64, 1, 1), "c96": (2, 3, 5, 96, 1, 1), "c96-nogate": (2, 2, 7, 96, 0, 1), "c256": (2, 2, 9, 256, 1, 1),
    "rows8200": (2, 4100, 2, 64, 1, 1),
}
POOL_SHAPES = {   # even grids; W/2 around wstep (16 fp32 / 32 bf16)
    "p2": (2, 2, 2, 64, 1, 1), "p30": (2, 2, 30, 64, 0, 1), "p32": (1, 4, 32, 64, 1, 0), "p34": (2, 2, 34, 64, 1, 1),
    "p66": (2, 4, 66, 64, 0, 0), "p128": (1, 2, 128, 256, 1, 1), "rows8200": (2, 8200, 2, 64, 1, 1),
}
OUTC_SHAPES = {   # id -> (B, H, W, C, gate, relu, K, bias); C = 8 / 64 / 256 give cpp = 1 .. 64 lanes per pixel over the two dtypes
    "k1": (2, 3, 17, 64, 1, 1, 1, 1), "k2": (2, 2, 33, 64, 0, 1, 2, 0), "k3": (1, 3, 65, 64, 1, 0, 3, 1), "k4": (2, 2, 129, 64, 1, 1, 4, 0),
    "c8": (2, 3, 70, 8, 1, 1, 2, 1), "c256": (2, 3, 5, 256, 1, 1, 3, 1), "c512": (1, 2, 3, 512, 0, 1, 4, 1), "w1": (2, 2, 1, 64, 1, 1, 2, 1),
    "rows8200": (2, 4100, 2, 64, 1, 1, 2, 1),
}


def apply_case(shape, T, seed, lattice=False):
    B, H, W, Cn, gate, relu = shape[:6]
    c = make_case(B, H, W, Cn, T, seed=seed, lattice=lattice)
    c.update(relu=relu, gate=gates(B, Cn, seed + 1, lattice) if gate else None)
    return c


def outc_case(name, T):
    """bf16: operands on a coarse binary grid, so that round_T(z) is the rounding of an exact value and cannot be taken the
    other way by the kernel's fp32 arithmetic; fp32: free operands (the rounding error of z is carried by the unit)."""
    shape = OUTC_SHAPES[name]
    Cn, K, bias = shape[3], shape[6], shape[7]
    c = apply_case(shape, T, seed=3000 + sum(map(ord, name)), lattice=T == BF16)
    g = gen(K + Cn)
    c["K"] = K
    c["wout"] = (torch.randint(-16, 17, (K, Cn), generator=g) / 16.0).float() if T == BF16 else torch.randn(K, Cn, generator=g) / Cn ** 0.5
    c["bias"] = torch.randn(K, generator=g) if bias else None
    return c


def plant_window_events(y, scale, shift, T):
    """Into the 2x2 windows of y (pre-activation scale*y + shift, ReLU on): equal positive values at every pair of positions,
    all-equal windows, ReLU zeros everywhere, and — bf16 — two values
    whose images differ by 3/8 ulp before the store and are equal after it, the larger one LATER in scan order (channel 3 is
    given scale 0.75, shift 3 for that). Returns y and the (scale, shift) to use. NaNs: plant_nans. Needs H/2 * W/2 >= 13 windows, C >= 16."""
    y, scale, shift = y.clone(), scale.clone(), shift.clone()
    B, H, W, Cn = y.shape
    pos = [(0, 0), (0, 1), (1, 0), (1, 1)]
    wins = [(h, w) for h in range(0, H - 1, 2) for w in range(0, W - 1, 2)]
    big = ((1.0 - shift) / scale).to(T)                                         # pre-activation about +1 in every channel
    k = 0
    for a in range(4):
        for b in range(a + 1, 4):                                              # 6 windows: a tie between positions a and b, the rest lower
            h, w = wins[k]; k += 1
            for q, (dh, dw) in enumerate(pos):
                y[:, h + dh, w + dw, :] = big if q in (a, b) else ((-1.0 - shift) / scale).to(T)
    h, w = wins[k]; k += 1
    for dh, dw in pos:
        y[:, h + dh, w + dw, :] = big                                           # all four equal and positive
    h, w = wins[k]; k += 1
    for dh, dw in pos:
        y[:, h + dh, w + dw, :] = ((-1.0 - shift) / scale).to(T)                # all four are ReLU zeros
    scale[3], shift[3] = 0.75, 3.0
    h, w = wins[k]; k += 1
    y[:, h:h + 2, w:w + 2, 3] = -8.0
    y[:, h, w, 3], y[:, h + 1, w, 3] = 1.0, 1.0 + 2.0 ** -7                     # 3.75 and 3.75 + 0.375 ulp(bf16): equal once stored as bf16
    return y, scale, shift


def plant_nans(y, first=9):
    """A NaN at each of the four positions, one per window, channels 8..15 of image 0, in windows first .. first + 3 (after the
    ReLU margin was enforced: a NaN has none)."""
    y = y.clone()
    B, H, W, Cn = y.shape
    wins = [(h, w) for h in range(0, H - 1, 2) for w in range(0, W - 1, 2)]
    for q, (dh, dw) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        h, w = wins[first + q]
        y[0, h + dh, w + dw, 8:16] = float("nan")
    return y


# --------------------------------------------------------------------------------------------------- sums and the stem
COLSUM_CASES = {  # id -> (segments, rows, cols, ld, accumulate, tmp: 1 given / 0 null)
    "r1": (1, 1, 64, 64, 0, 1), "r255": (3, 255, 63, 63, 1, 1), "r256": (1, 256, 65, 65, 0, 1), "r257": (3, 257, 1, 1, 0, 1),
    "r300": (1, 300, 64, 80, 1, 1), "r300-notmp": (3, 300, 65, 65, 0, 0), "r300-ld": (3, 300, 63, 100, 0, 1),
    "r65600": (1, 65600, 3, 3, 0, 1), "r1000-ld": (3, 1000, 64, 70, 1, 1),
}
PARTIAL_CASES = {"rps1": (5, 65, 1), "rps7": (300, 63, 7), "rps128": (300, 64, 128), "rps128-ragged": (257, 1, 128)}   # rows, cols, rps


def colsum_case(name):
    seg, rows, cols, ld, acc, tmp = COLSUM_CASES[name]
    g = gen(sum(map(ord, name)))
    part = torch.randn(seg, rows, cols, generator=g) + 0.5 * torch.randn(seg, 1, cols, generator=g)
    return dict(part=part, out0=torch.randn(seg, cols, generator=g), seg=seg, rows=rows, cols=cols, ld=ld, acc=acc, tmp=tmp)


SUMHW_CASES = {  # id -> (B, H, W, C, factor)
    "hw1": (2, 1, 1, 64, 1.0), "hw63": (2, 7, 9, 64, 1.0 / 63), "hw64": (1, 8, 8, 192, 0.3), "hw65": (2, 5, 13, 64, 1.0),
    "hw1000": (2, 25, 40, 192, 1e-3),
}
STEM_CASES = {   # id -> (B, H, W): W/2 in {1, 31, 32, 33, 70}, H/2 in {1, 9}; B*Ho = 27 is no multiple of 8 and its blocks of 8 rows straddle images
    "wo1": (3, 18, 2), "wo31": (2, 2, 62), "wo32": (1, 2, 64), "wo33": (3, 18, 66), "wo70": (2, 18, 140),
}


def stem_case(name, T, representable=True):
    B, H, W = STEM_CASES[name]
    g = gen(sum(map(ord, name)))
    x, w = torch.randn(B, H, W, generator=g), 0.1 * torch.randn(64, 49, generator=g)
    if representable:
        x, w = x.to(T).float(), w.to(T).float()
    return dict(x=x, w=w, dy=torch.randn(B, H // 2, W // 2, 64, generator=g).to(T), B=B, H=H, W=W)


def rand_act(shape, T, seed, offset=0.3):
    g = gen(seed)
    return (torch.randn(shape, generator=g) + offset * torch.randn(shape[-1], generator=g)).to(T)


def trunc_bf16(x):
    """fp32 -> bf16 by truncation (the wrong store, for the sensitivity test)."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


# ---------------------------------------------------------------------------------------------------- bilinear resizes
# id -> ((Hi, Wi), (Ho, Wo)): the 2x and the ragged up-sampling, shrinking (scale above 1: the adjoint's window comes from
# divisions), equal sizes (the identity, bit for bit), one-pixel sources and destinations, the decoder's one-pixel resizes
RESIZE_CASES = {
    "up8": ((8, 8), (64, 64)), "up-ragged": ((5, 7), (13, 30)), "up12x20": ((12, 20), (96, 160)),
    "down-ragged": ((13, 30), (5, 7)), "down8": ((64, 64), (8, 8)), "same": ((6, 9), (6, 9)),
    "src1x1": ((1, 1), (5, 7)), "src1xW": ((1, 6), (4, 9)), "srcHx1": ((6, 1), (9, 4)), "dst1x1": ((5, 7), (1, 1)),
    "plus1": ((24, 46), (25, 47)), "plus1w": ((8, 8), (8, 9)),
}

# float32 floor of tests/pointwise_ref.resize_fwd / resize_bwd over these cases (tests/test_pointwise_ref_host.py asserts it),
# rounded up, and the K of the resizes: twice the largest, as the floor is above 1
RESIZE_FLOOR = {"resize_fwd": 91.19, "resize_bwd": 110.52}
RESIZE_K = 221.04


def resize_case(name, T, B=2, Cn=64, seed=300):
    """x [B][Hi][Wi][C] and the upstream gradient g [B][Ho][Wo][C], stored in T: magnitudes in [0.5, 1.5) with random signs.
    The bounded range is what makes the rule's unit meaningful here: a float32 src moves a tap's weight by about 2^-24 * src
    whatever the weight's own size, an error of that times |x1 - x0|, while U = sum |w * x| can be as small as the smallest
    |x| among the taps; with normal deviates the float32 floor itself is then heavy-tailed (100 and more on these cases)."""
    (hi, wi), (ho, wo) = RESIZE_CASES[name]
    g = gen(seed + sorted(RESIZE_CASES).index(name))

    def draw(*shape):
        sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        return (sign * (0.5 + torch.rand(shape, generator=g))).to(T)
    return {"x": draw(B, hi, wi, Cn), "g": draw(B, ho, wo, Cn), "in": (hi, wi), "out": (ho, wo)}
