"""Numpy restatement of csrc/augment.hip: aug_hash64, the table draw, the D4 ops and the apply arithmetic, in float32,
rounding for rounding. Shared by the host and the GPU tests of the augmentation; not a test module itself."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MIX1 = np.uint64(0xBF58476D1CE4E5B9)
MIX2 = np.uint64(0x94D049BB133111EB)
STEP_MUL = 0xD1B54A32D192ED03
NOISE_STREAM = 0x5851F42D4C957F2D
MASK64 = (1 << 64) - 1
ZS = np.float32(float.fromhex("0x1.bb67aep-16"))
INVERSE = (0, 1, 2, 3, 4, 6, 5, 7)


def hash64(key: int, i) -> np.ndarray:
    """aug_hash64(key, i) for an array of counters i: uint64 arithmetic with wrap-around (numpy arrays wrap silently)."""
    i = np.atleast_1d(np.asarray(i)).astype(np.uint64)
    z = np.full(i.shape, key & MASK64, dtype=np.uint64) + GOLDEN * (i + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * MIX1
    z = (z ^ (z >> np.uint64(27))) * MIX2
    return z ^ (z >> np.uint64(31))


def hash64_int(key: int, i: int) -> int:
    return int(hash64(key, [i])[0])


def key_seed(seed: int, rank: int) -> int:
    return hash64_int(seed, rank)


def noise_seed(seed: int, rank: int, step: int) -> int:
    return hash64_int(key_seed(seed, rank) ^ NOISE_STREAM, step)


def uniform(h) -> np.ndarray:
    """u(h) = (float)(h >> 8) * 2^-24 of the 32-bit words h: exact, in [0, 1)."""
    return (np.asarray(h, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def draw(seed: int, step: int, n: int, ops_mask: int, gain, bias, sigma) -> np.ndarray:
    """The table insar_aug_draw(seed, step, n, ops_mask, ...) fills: int32 [n, 4] = {op, bits of gain, bias, sigma}."""
    key = (seed ^ ((step * STEP_MUL) & MASK64)) & MASK64
    h = (hash64(key, np.arange(4 * n)) >> np.uint64(32)).reshape(n, 4)
    bits = [b for b in range(8) if (ops_mask >> b) & 1]
    table = np.zeros((n, 4), dtype=np.int32)
    table[:, 0] = np.asarray(bits, dtype=np.int32)[(h[:, 0] % np.uint64(len(bits))).astype(np.int64)]
    for col, (lo, hi) in enumerate((gain, bias, sigma), start=1):
        lo, hi = np.float32(lo), np.float32(hi)
        d = np.float32(hi - lo)
        prod = (d * uniform(h[:, col])).astype(np.float32)
        table[:, col] = (lo + prod).astype(np.float32).view(np.int32)
    return table


def d4(a: np.ndarray, op: int) -> np.ndarray:
    """D4 op on the last two axes of `a`."""
    b = np.swapaxes(a, -1, -2) if op & 4 else a
    if op & 2:
        b = b[..., ::-1, :]
    if op & 1:
        b = b[..., :, ::-1]
    return b


def noise_z(seed: int, lin) -> np.ndarray:
    """z of the output elements `lin`: the sum of the four 16-bit fields of the hash, centred, times ZS (one rounding)."""
    h = hash64(seed, lin)
    m = np.uint64(0xffff)
    S = ((h & m) + ((h >> np.uint64(16)) & m) + ((h >> np.uint64(32)) & m) + (h >> np.uint64(48))).astype(np.int64)
    return (S - 131070).astype(np.float32) * ZS


def make_table(ops, gains, biases, sigmas) -> np.ndarray:
    t = np.zeros((len(ops), 4), dtype=np.int32)
    t[:, 0] = np.asarray(ops, dtype=np.int64).astype(np.int32)
    for col, v in enumerate((gains, biases, sigmas), start=1):
        t[:, col] = np.asarray(v, dtype=np.float32).view(np.int32)
    return t


def apply(x, m, table: np.ndarray, seed: int = 0):
    """(xo, mo) of insar_aug_apply: x float32 [n, C, H, W] or None, m integer [n, H, W] or None, table int32 [n, 4]."""
    xo = mo = None
    f = table.view(np.float32)
    if x is not None:
        n, C, H, W = x.shape
        xo = np.empty_like(x)
        for s in range(n):
            op = int(table[s, 0]) & (7 if H == W else 3)
            t = (f[s, 1] * d4(x[s], op)).astype(np.float32)
            t = (t + f[s, 2]).astype(np.float32)
            if f[s, 3] != 0:
                lin = np.arange(s * C * H * W, (s + 1) * C * H * W, dtype=np.uint64)
                nz = (f[s, 3] * noise_z(seed, lin).reshape(C, H, W)).astype(np.float32)
                t = (t + nz).astype(np.float32)
            xo[s] = t
    if m is not None:
        n, H, W = m.shape
        mo = np.empty(m.shape, dtype=np.int64)
        for s in range(n):
            mo[s] = d4(m[s], int(table[s, 0]) & (7 if H == W else 3)).astype(np.int64)
    return xo, mo
