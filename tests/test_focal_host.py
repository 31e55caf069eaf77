"""CPU-only: the numpy restatement of the focal operations (tests/focal_ref.py) pinned by an evaluator in Python integers that
runs a direct 2-D double loop and makes no use of separability; the tap builders; the properties README.md promises (ties
towards +infinity, a constant raster reproduced under any validity pattern, the lower median, no value invented); a derived
error bound; and the module surface: every argument refusal of insar_unet_ca_amd/focal.py, the exports and detect's keyword."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import focal as fc
from insar_unet_ca_amd._lib import InsarError
from insar_unet_ca_amd.hysteresis import ordered_u32
from insar_unet_ca_amd.zonal import quantise_scalar
from tests import focal_ref as ref

Q_LIMIT = (1 << 31) - 1


# ---- the independent evaluator ----------------------------------------------------------------------------------------------------
def _is_valid(r, valid, nodata, y, x):
    H, W = r.shape
    if not (0 <= y < H and 0 <= x < W):
        return False
    if valid is not None and valid[y, x] == 0:
        return False
    v = r[y, x]
    if nodata is not None and v == r.dtype.type(nodata):
        return False
    return bool(np.isfinite(v)) if r.dtype == np.float32 else True


def evaluate_smooth(r, taps, scale, valid, nodata, min_coverage, keep_invalid, fill):
    """One plane, Python integers, the full 2-D window per output pixel."""
    H, W = r.shape
    k = [int(t) for t in taps]
    R, S = len(k) // 2, sum(k)
    T = max(1, math.ceil(Fraction(min_coverage) * S * S))
    out = np.zeros((H, W), dtype=r.dtype)
    ok = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            N = D = 0
            for j in range(-R, R + 1):
                for i in range(-R, R + 1):
                    if _is_valid(r, valid, nodata, y + j, x + i):
                        w = k[j + R] * k[i + R]
                        q = quantise_scalar(float(r[y + j, x + i]), scale) if r.dtype == np.float32 else int(r[y + j, x + i])
                        N += w * q
                        D += w
            good = D >= T and (not keep_invalid or _is_valid(r, valid, nodata, y, x))
            ok[y, x] = good
            if good:
                q_out = math.floor(Fraction(N, D) + Fraction(1, 2))         # ties towards +infinity
                out[y, x] = np.float32(np.float64(q_out) / np.float64(scale)) if r.dtype == np.float32 else q_out
            else:
                out[y, x] = ref.QNAN if r.dtype == np.float32 else fill
    return out, ok


def _same(got, want, what=""):
    assert got[1].dtype == np.uint8 and got[0].dtype == want[0].dtype, what
    assert np.array_equal(got[1], want[1]), f"{what}: valid plane"
    assert got[0].tobytes() == want[0].tobytes(), f"{what}: values"


def _random_case(rng, H, W, dtype):
    if dtype == np.float32:
        r = (rng.standard_normal((H, W)) * 3).astype(np.float32)
        r[rng.random((H, W)) < 0.1] = np.nan
        r[rng.random((H, W)) < 0.05] = np.inf
        r[rng.random((H, W)) < 0.05] = -7.5
    elif dtype == np.uint8:
        r = rng.integers(0, 256, (H, W)).astype(np.uint8)
    else:
        r = rng.integers(-(1 << 31), 1 << 31, (H, W)).astype(np.int32)
    valid = (rng.random((H, W)) > 0.3).astype(np.uint8) * 3
    return r, valid


@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.int32])
def test_restatement_against_python_integers(dtype):
    rng = np.random.default_rng(11)
    for n, (H, W) in enumerate(((1, 1), (1, 7), (5, 3), (12, 12), (9, 11))):
        r, valid = _random_case(rng, H, W, dtype)
        nodata = {np.float32: -7.5, np.uint8: 17, np.int32: int(r[0, 0])}[dtype]
        taps = [[1], [1, 2, 1], [0, 3, 1], [5, 0, 2, 1, 7], [1] * 7, fc.gaussian_taps(1.5)][n % 6]
        for valid_ in (None, valid):
            for nodata_ in (None, nodata):
                for cov, keep in ((0.0, True), (0.5, False), (1.0, True), (0.3, False)):
                    scale = 2 ** 16 if dtype != np.float32 or n % 2 else 1000.0
                    kw = dict(scale=scale, valid=valid_, nodata=nodata_, min_coverage=cov, keep_invalid=keep, fill=9)
                    _same(ref.smooth(r, taps, **kw), evaluate_smooth(r, taps, **kw), f"{dtype.__name__} {H}x{W} {kw}")


def test_restatement_at_both_extremes_of_int64_use():
    """Every pixel clamped to +-(2^31 - 1) under box taps of R = 15 whose sum sits at the 4096 limit: |A| and |N| as large as they get."""
    taps = np.full(31, 132, dtype=np.int64)
    taps[15] += 4096 - int(taps.sum())
    assert taps.sum() == 4096
    for sign in (1.0, -1.0):
        r = np.full((12, 12), sign * 1e30, dtype=np.float32)
        got = ref.smooth(r, taps)
        _same(got, evaluate_smooth(r, taps, 2 ** 16, None, None, 0.0, True, 0), f"sign {sign}")
        assert (got[0] == np.float32(sign * Q_LIMIT / 65536.0)).all()
    ri = np.full((12, 12), -(1 << 31), dtype=np.int32)                  # int32 rasters reach one further down
    _same(ref.smooth(ri, taps), evaluate_smooth(ri, taps, 2 ** 16, None, None, 0.0, True, 0), "int32 minimum")
    mixed = np.where(np.indices((12, 12)).sum(0) % 2, 1e30, -1e30).astype(np.float32)
    _same(ref.smooth(mixed, taps), evaluate_smooth(mixed, taps, 2 ** 16, None, None, 0.0, True, 0), "alternating signs")


def test_quantisation_is_zonal_s_rule():
    v = np.array([0.0, 1.0, -1.0, 0.5 / 65536, 1.5 / 65536, -0.5 / 65536, 2.5 / 65536, 1e30, -1e30, 32767.99999, 3.3e-7], dtype=np.float32)
    for scale in (2 ** 16, 1000.0, 0.37):
        assert ref.quantise(v, scale).tolist() == [quantise_scalar(float(x), scale) for x in v]


# ---- tap builders --------------------------------------------------------------------------------------------------------------------
def test_tap_builders():
    assert fc.box_taps(0).tolist() == [1] and fc.box_taps(3).tolist() == [1] * 7 and fc.box_taps(15).sum() == 31
    for sigma, radius, total in ((1.5, None, 4096), (0.3, None, 4096), (5.0, None, 4096), (2.0, 3, 1000), (4.0, 15, 4096), (1.0, 0, 7),
                                 (0.01, None, 4096)):
        t = fc.gaussian_taps(sigma, radius, total) if radius is not None else fc.gaussian_taps(sigma, total=total)
        R = radius if radius is not None else math.ceil(3 * sigma)
        assert t.dtype == np.int32 and len(t) == 2 * R + 1                          # R from sigma
        assert t.tolist() == t[::-1].tolist() and int(t.sum()) == total and (t >= 0).all()
        i = np.arange(-R, R + 1, dtype=np.float64)
        w = np.exp(-i * i / (2.0 * sigma * sigma))
        side = np.floor(w / w.sum() * total)
        assert np.abs(t[:R] - side[:R]).max(initial=0) <= 1                          # floor of the share (one ulp of the sum aside)
        assert t[R] == total - 2 * t[:R].sum() >= t.max()                            # the remainder sits on the centre tap
    assert fc.gaussian_taps(1.5).tolist() == fc.gaussian_taps(1.5, 5, 4096).tolist()
    for call, msg in ((lambda: fc.box_taps(16), "box_taps: radius=16"), (lambda: fc.box_taps(-1), "box_taps: radius=-1"),
                      (lambda: fc.box_taps(1.0), "box_taps: radius=1.0"),
                      (lambda: fc.gaussian_taps(0.0), "gaussian_taps: sigma=0.0"), (lambda: fc.gaussian_taps(float("nan")), "sigma=nan"),
                      (lambda: fc.gaussian_taps("1"), "sigma='1'"), (lambda: fc.gaussian_taps(True), "sigma=True"),
                      (lambda: fc.gaussian_taps(5.1), r"ceil\(3 sigma\) = 16 exceeds 15"),
                      (lambda: fc.gaussian_taps(1.0, 16), "radius=16"), (lambda: fc.gaussian_taps(1.0, 2, 4097), "total=4097"),
                      (lambda: fc.gaussian_taps(1.0, 2, 0), "total=0")):
        with pytest.raises(InsarError, match=msg):
            call()
    assert fc.check_taps("t", [0, 0, 5]).tolist() == [0, 0, 5] and fc.check_taps("t", (4096,)).tolist() == [4096]
    for taps, msg in (([1, 2], "2 R \\+ 1 integers"), ([], "2 R \\+ 1 integers"), ([1] * 33, "2 R \\+ 1 integers"), ([1.0, 2.0, 1.0], "integers"),
                      ([[1, 2, 1]], "1-D"), ([1, -1, 1], "negative"), ([0, 0, 0], "sum to 0"), ([2000, 2000, 97], "sum to 4097"),
                      (torch.ones(3), "host sequence"), ("121", "host sequence")):
        with pytest.raises(InsarError, match="who: taps.*" + msg):
            fc.check_taps("who", taps)
    assert [fc.coverage_threshold(c, 4096) for c in (0.0, 0.5, 1.0)] == [1, 1 << 23, 1 << 24]
    assert fc.coverage_threshold(0.1, 3) == 1 and fc.coverage_threshold(0.12, 3) == 2
    assert [ref.threshold(c, s) for c, s in ((0.0, 7), (0.5, 16), (1.0, 4096), (0.12, 3))] == [1, 128, 1 << 24, 2]


# ---- properties ------------------------------------------------------------------------------------------------------------------------
def test_derived_bound_on_all_valid_data():
    """All valid: the result lies within 1 / scale plus one float32 ulp of the float64 weighted mean under the same integer
    taps: half a unit of 1 / scale from quantising the inputs (a convex combination of errors <= 1/2), half from rounding the
    quotient, and the last rounding to float32. The float64 mean itself carries (2R + 1)^2 roundings of 2^-53 relative to the
    largest |v|, which is added as such. No measured number."""
    rng = np.random.default_rng(5)
    for taps, scale in ((fc.gaussian_taps(1.5), 2 ** 16), (fc.box_taps(3), 2 ** 16), ([3, 0, 1, 9, 2], 1000.0), (fc.gaussian_taps(4.0, 15), 2 ** 10)):
        r = (rng.standard_normal((40, 37)) * 20).astype(np.float32)
        out, ok = ref.smooth(r, taps, scale=scale)
        assert ok.all()
        k = np.asarray(taps, dtype=np.float64)
        R = len(k) // 2
        num = np.zeros(r.shape)
        den = np.zeros(r.shape)
        rp = np.pad(r.astype(np.float64), R)
        mp = np.pad(np.ones(r.shape), R)
        for j in range(2 * R + 1):
            for i in range(2 * R + 1):
                num += k[j] * k[i] * rp[j:j + 40, i:i + 37]
                den += k[j] * k[i] * mp[j:j + 40, i:i + 37]
        mean = num / den
        bound = 1.0 / scale + np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64) + len(k) ** 2 * 2.0 ** -53 * np.abs(r).max()
        err = np.abs(out.astype(np.float64) - mean)
        print(f"taps sum {int(k.sum())}, scale {scale}: worst error / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()


def test_exact_ties_round_towards_plus_infinity():
    # two valid pixels under box taps: the mean of q = a and q = b with a + b odd is an exact tie
    for a, b, want in ((1, 2, 2), (-1, -2, -1), (-3, 0, -1), (-1, 0, 0), (3, 0, 2), (-2 ** 31 + 1, -2 ** 31 + 2, -2 ** 31 + 2)):
        r = np.array([[a, b]], dtype=np.int32)
        out, ok = ref.smooth(r, [1, 1, 0], keep_invalid=False)              # taps at offsets -1 and 0
        assert ok.tolist() == [[1, 1]] and out[0, 1] == want and out[0, 0] == a, (a, b)
        e, _ = evaluate_smooth(r, [1, 1, 0], 2 ** 16, None, None, 0.0, False, 0)
        assert e[0, 1] == want
        f = (r.astype(np.float64) / 65536.0).astype(np.float32)             # the same ties behind the quantisation
        outf, _ = ref.smooth(f, [1, 1, 0])
        assert outf[0, 1] == np.float32(want / 65536.0)
    # what is no tie rounds to nearest on both sides of zero: -0.75 -> -1, -0.25 -> 0
    out, _ = ref.smooth(np.array([[-1, -1, -1, 0]], dtype=np.int32), [1, 1, 1, 1, 0, 0, 0])
    assert out[0, 3] == -1
    out, _ = ref.smooth(np.array([[0, 0, 0, -1]], dtype=np.int32), [1, 1, 1, 1, 0, 0, 0])
    assert out[0, 3] == 0


def test_a_constant_raster_comes_back_as_its_own_quantisation():
    rng = np.random.default_rng(8)
    for value, scale in ((0.3, 2 ** 16), (-1234.56789, 1000.0), (1e30, 2 ** 16), (-0.0, 2 ** 16)):
        r = np.full((3, 23, 19), value, dtype=np.float32)
        valid = (rng.random((23, 19)) > 0.5).astype(np.uint8)
        for taps in (fc.gaussian_taps(1.5), fc.box_taps(15), [0, 0, 7, 1, 0]):
            for keep in (True, False):
                out, ok = ref.smooth(r, taps, scale=scale, valid=valid, keep_invalid=keep)
                q = quantise_scalar(value, scale)
                assert (out[ok != 0] == np.float32(np.float64(q) / np.float64(scale))).all() and np.isnan(out[ok == 0]).all()
                assert (ok[:, valid != 0] == 1).all()
    ri = np.full((9, 9), -77, dtype=np.int32)
    out, ok = ref.smooth(ri, fc.gaussian_taps(2.0), valid=(rng.random((9, 9)) > 0.5).astype(np.uint8), keep_invalid=False, fill=5)
    assert set(np.unique(out).tolist()) <= {-77, 5} and (out[ok != 0] == -77).all()


def test_a_single_centre_tap_gives_the_quantised_input():
    r = ref.speckle((17, 13), 3)
    for taps in ([1], [0, 9, 0], [0, 0, 4096, 0, 0]):
        out, ok = ref.smooth(r, taps, scale=1000.0)
        m = np.isfinite(r)
        assert np.array_equal(ok != 0, m)
        want = (ref.quantise(r, 1000.0).astype(np.float64) / 1000.0).astype(np.float32)
        assert out[m].tobytes() == want[m].tobytes() and np.isnan(out[~m]).all()
    u = np.arange(200, dtype=np.uint8).reshape(10, 20)
    assert np.array_equal(ref.smooth(u, [0, 3, 0])[0], u)


def test_the_lower_median_is_an_input_value():
    rng = np.random.default_rng(2)
    r = rng.standard_normal((14, 15)).astype(np.float32)
    for radius in (1, 2, 3):
        out, ok = ref.rank(r, "median", radius)
        n = 2 * radius + 1
        win = np.lib.stride_tricks.sliding_window_view(r, (n, n)).reshape(14 - n + 1, 15 - n + 1, n * n)
        inner = out[radius:14 - radius, radius:15 - radius]
        assert np.array_equal(inner, np.median(win, axis=-1)) and ok.all()          # odd all-valid windows
    holes = r.copy()
    holes[rng.random(r.shape) < 0.4] = np.nan
    holes[3, 4], holes[3, 5] = -0.0, 0.0
    for op, radius in (("median", 1), ("median", 3), ("min", 2), ("max", 2), ("min", 15)):
        out, ok = ref.rank(holes, op, radius, keep_invalid=False)
        m = np.isfinite(holes)
        for y, x in np.ndindex(*r.shape):
            ys, xs = slice(max(y - radius, 0), y + radius + 1), slice(max(x - radius, 0), x + radius + 1)
            vals = holes[ys, xs][m[ys, xs]]
            assert ok[y, x] == (len(vals) > 0)
            if len(vals):
                keys = np.sort(ordered_u32(vals))                                   # -0.0 directly below 0.0
                want = {"min": keys[0], "max": keys[-1], "median": keys[(len(keys) - 1) // 2]}[op]
                assert ordered_u32(out[y, x:x + 1])[0] == want                      # the exact bit pattern of an input pixel
    two = np.array([[5, 1, 9, 3]], dtype=np.uint8)                                  # even n: the lower of the two middle values
    assert ref.rank(two, "median", 1, valid=np.array([[1, 1, 0, 1]], dtype=np.uint8), keep_invalid=False)[0].tolist() == [[1, 1, 1, 3]]
    out, ok = ref.rank(two, "median", 1, min_count=3, fill=200)
    assert out.tolist() == [[200, 5, 3, 200]] and ok.tolist() == [[0, 1, 1, 0]]


def test_gradient_stencils_by_hand():
    nan = np.nan
    r = np.array([[1.0, 4.0, 9.0, nan, 25.0, 36.0, nan, 64.0, nan]], dtype=np.float32)
    out, ok = ref.gradient(r, spacing=(1.0, 0.5))
    gx = out[1, 0]
    #          fwd  central  bwd  centre invalid  fwd   bwd   invalid  isolated  invalid
    want = [6.0, 8.0, 10.0, nan, 22.0, 22.0, nan, nan, nan]
    assert np.array_equal(gx, np.array(want, dtype=np.float32), equal_nan=True)
    assert np.isnan(out[0]).all() and not ok.any()                                  # one row: no y neighbour at all
    filled, _ = ref.gradient(r, spacing=(1.0, 0.5), keep_invalid=False)
    assert filled[1, 0, 3] == np.float32((25.0 - 9.0) * 1.0) and np.isnan(filled[1, 0, 8])      # both neighbours of the hole are valid
    col, okc = ref.gradient(r.T.copy(), spacing=(0.5, 1.0))
    assert np.array_equal(col[0][:, 0], gx, equal_nan=True) and np.isnan(col[1]).all()
    sq = np.arange(12, dtype=np.float32).reshape(3, 4) ** 2
    out, ok = ref.gradient(sq, spacing=(2.0, 1.0))
    assert ok.all() and out[0, 1, 1] == np.float32((81.0 - 1.0) * 0.25) and out[1, 1, 1] == np.float32((36.0 - 16.0) * 0.5)


# ---- the module surface -----------------------------------------------------------------------------------------------------------------
def test_exports():
    for name in ("smooth_raster", "rank_filter", "gradient_raster", "box_taps", "gaussian_taps", "focal_tile"):
        assert name in iu.__all__ and getattr(iu, name) is getattr(fc, name)
    TH, TW = fc.focal_tile(0)
    assert TH >= 1 and TW >= 1 and all(fc.focal_tile(r) == (TH, TW) or min(fc.focal_tile(r)) >= 1 for r in (1, 7, 15))
    with pytest.raises(InsarError, match="focal_tile: radius=16"):
        fc.focal_tile(16)


def _refused(fn, who, cases, *lead):
    for kw, msg in cases:
        kw = dict(kw)
        raster = kw.pop("raster")
        with pytest.raises(InsarError, match=who + ": .*" + msg):
            fn(raster, *[kw.pop(n) for n in lead], **kw)


def test_smooth_raster_refusals():
    r = torch.zeros(8, 9)
    t = [1, 2, 1]
    u8 = r.to(torch.uint8)
    _refused(fc.smooth_raster, "smooth_raster", [
        (dict(raster=r.double(), taps=t), "raster must be float32 or uint8 or int32"),
        (dict(raster=r[None, None], taps=t), "raster must be 2-D"),
        (dict(raster=r.t(), taps=t), "raster must be contiguous"),
        (dict(raster=np.zeros((3, 3)), taps=t), "raster must be a torch tensor"),
        (dict(raster=torch.zeros(0, 4), taps=t), "need H, W >= 1"),
        (dict(raster=torch.empty((1 << 16, 1 << 15), dtype=torch.uint8, device="meta"), taps=t), r"H \* W < 2\^31"),
        (dict(raster=torch.empty((65536, 1, 1), dtype=torch.uint8, device="meta"), taps=t), "1..65535 planes"),
        (dict(raster=r, taps=[1, 2]), "taps: a 1-D sequence of 2 R \\+ 1 integers"),
        (dict(raster=r, taps=[1, -2, 1]), "negative"),
        (dict(raster=r, taps=[4096, 1, 0]), "sum to 4097"),
        (dict(raster=r, taps=t, scale=0.0), "scale=0.0: a positive finite number"),
        (dict(raster=r, taps=t, scale=float("inf")), "scale=inf"),
        (dict(raster=u8, taps=t, scale=256.0), "scale=256.0: a torch.uint8 raster is taken as it is"),
        (dict(raster=r, taps=t, valid=torch.ones(8, 9)), "valid must be a contiguous 2-D uint8"),
        (dict(raster=r, taps=t, valid=torch.ones(9, 8, dtype=torch.uint8)), r"valid \(9, 8\): expected \(8, 9\)"),
        (dict(raster=r[None].expand(2, 8, 9).contiguous(), taps=t, valid=torch.ones(2, 8, 9, dtype=torch.uint8)), "valid must be a contiguous 2-D"),
        (dict(raster=r, taps=t, nodata=float("nan")), "nodata is NaN"),
        (dict(raster=r, taps=t, nodata="x"), "nodata='x'"),
        (dict(raster=u8, taps=t, nodata=300), "nodata=300 is no value"),
        (dict(raster=u8, taps=t, nodata=1.5), "nodata=1.5 is no value"),
        (dict(raster=r, taps=t, min_coverage=1.5), "min_coverage=1.5: a number in 0..1"),
        (dict(raster=r, taps=t, min_coverage=float("nan")), "min_coverage=nan"),
        (dict(raster=r, taps=t, keep_invalid=1), "keep_invalid=1: True or False"),
        (dict(raster=r, taps=t, return_valid=None), "return_valid=None"),
        (dict(raster=r, taps=t, fill=1), "fill=1: invalid float32 outputs are NaN"),
        (dict(raster=u8, taps=t, fill=256), "fill=256: a value of a torch.uint8 raster"),
        (dict(raster=r.to(torch.int32), taps=t, fill=1.0), "fill=1.0"),
        (dict(raster=r, taps=t, out=torch.zeros(8, 8)), "out must be a contiguous torch.float32 tensor \\(8, 9\\)"),
        (dict(raster=r, taps=t, out=torch.zeros(8, 9, dtype=torch.int32)), "out must be"),
        (dict(raster=r, taps=t, out=r), "shares no memory with the raster"),
        (dict(raster=r, taps=t, out=np.zeros((8, 9), dtype=np.float32)), "out must be"),
        (dict(raster=r, taps=t), r"raster must be a ROCm tensor \(no CPU fallback\)"),              # every other check passed
    ], "taps")
    big = torch.zeros(3, 8, 9)
    with pytest.raises(InsarError, match="shares no memory"):
        fc.smooth_raster(big[1], t, out=big[:2].view(2, 8, 9)[1])


def test_rank_filter_refusals():
    r = torch.zeros(8, 9)
    _refused(fc.rank_filter, "rank_filter", [
        (dict(raster=r.double(), op="min", radius=1), "raster must be float32 or uint8 or int32"),
        (dict(raster=r, op="mean", radius=1), "op='mean': 'min', 'max' or 'median'"),
        (dict(raster=r, op=0, radius=1), "op=0"),
        (dict(raster=r, op="min", radius=0), "radius=0: an integer in 1..15"),
        (dict(raster=r, op="max", radius=16), "radius=16: an integer in 1..15"),
        (dict(raster=r, op="median", radius=4), "radius=4: an integer in 1..3"),
        (dict(raster=r, op="median", radius=1.0), "radius=1.0"),
        (dict(raster=r, op="median", radius=1, min_count=0), "min_count=0: an integer in 1..9"),
        (dict(raster=r, op="median", radius=1, min_count=10), "min_count=10"),
        (dict(raster=r, op="min", radius=1, nodata=float("nan")), "nodata is NaN"),
        (dict(raster=r, op="min", radius=1, valid=torch.ones(8, 9)), "valid must be"),
        (dict(raster=r, op="min", radius=1, keep_invalid="yes"), "keep_invalid='yes'"),
        (dict(raster=r, op="min", radius=1, fill=3), "fill=3"),
        (dict(raster=r, op="min", radius=1, out=r), "shares no memory"),
        (dict(raster=r, op="min", radius=1), r"raster must be a ROCm tensor \(no CPU fallback\)"),
    ], "op", "radius")
    with pytest.raises(TypeError):                                              # raw values: there is no quantisation and no scale
        fc.rank_filter(r, "min", 1, scale=2.0)


def test_gradient_raster_refusals():
    r = torch.zeros(8, 9)
    _refused(fc.gradient_raster, "gradient_raster", [
        (dict(raster=r.to(torch.int32)), "raster must be float32"),
        (dict(raster=r.to(torch.uint8)), "raster must be float32"),
        (dict(raster=r, spacing=1.0), "spacing=1.0: \\(dy, dx\\)"),
        (dict(raster=r, spacing=(1.0, 0.0)), "spacing=\\(1.0, 0.0\\)"),
        (dict(raster=r, spacing=(1.0, -2.0)), "positive finite"),
        (dict(raster=r, spacing=(float("nan"), 1.0)), "positive finite"),
        (dict(raster=r, spacing=(1.0, 2.0, 3.0)), "\\(dy, dx\\)"),
        (dict(raster=r, spacing=(1e-40, 1.0)), "leaves the float32 range"),
        (dict(raster=r, spacing=(1.0, 1e300)), "leaves the float32 range"),
        (dict(raster=r, nodata=float("nan")), "nodata is NaN"),
        (dict(raster=r, valid=torch.ones(8, 9)), "valid must be"),
        (dict(raster=r, keep_invalid=0), "keep_invalid=0"),
        (dict(raster=r, out=torch.zeros(8, 9)), "out must be a contiguous torch.float32 tensor \\(2, 8, 9\\)"),
        (dict(raster=torch.zeros(3, 8, 9), out=torch.zeros(2, 3, 8, 9)), "\\(3, 2, 8, 9\\)"),
        (dict(raster=r), r"raster must be a ROCm tensor \(no CPU fallback\)"),
    ])
    big = torch.zeros(3, 8, 9)
    with pytest.raises(InsarError, match="shares no memory"):
        fc.gradient_raster(big[0], out=big[:2])
    assert fc.reciprocal_spacing("g", (2.0, 4.0)) == (np.float32(0.5), np.float32(0.25), np.float32(0.25), np.float32(0.125))


def test_entry_points_check_before_they_touch_a_device():
    import ctypes as C
    from insar_unet_ca_amd import _lib
    taps = (C.c_int32 * 3)(1, 2, 1)
    buf = (C.c_float * 16)()
    out = (C.c_float * 32)()
    a, o = C.addressof(buf), C.addressof(out)
    F = _lib.ZONAL_F32
    smooth = lambda **k: _lib.call("insar_focal_smooth", k.get("raster", a), k.get("elem", F), k.get("planes", 1), k.get("H", 4), k.get("W", 4),
                                   k.get("taps", taps), k.get("radius", 1), k.get("scale", 1.0), 0, 0.0, None, k.get("threshold", 1), 1,
                                   k.get("fill", 0), k.get("out", o), None, None)
    for kw, msg in ((dict(raster=None), "null pointer \\(raster\\)"), (dict(out=a), "out is the raster itself"), (dict(elem=7), "element type 7"),
                    (dict(H=0), "empty raster"), (dict(H=1 << 16, W=1 << 15), "2\\^31 pixels or more"), (dict(planes=0), "planes 0"),
                    (dict(taps=None), "null pointer \\(taps\\)"), (dict(radius=16), "radius 16"), (dict(taps=(C.c_int32 * 3)(1, -1, 1)), "negative"),
                    (dict(taps=(C.c_int32 * 3)(4096, 1, 0)), "sum to 4097"), (dict(taps=(C.c_int32 * 3)(0, 0, 0)), "sum to 0"),
                    (dict(threshold=0), "threshold 0"), (dict(threshold=17), "threshold 17 outside 1..16"), (dict(scale=0.0), "scale 0"),
                    (dict(elem=_lib.ZONAL_U8, fill=256), "fill 256"), (dict(raster=a + 2), "not 4-byte aligned")):
        with pytest.raises(InsarError, match="insar_focal_smooth: .*" + msg):
            smooth(**kw)
    rank = lambda op, radius, min_count=1: _lib.call("insar_focal_rank", a, F, 1, 4, 4, op, radius, 0, 0.0, None, min_count, 1, 0, o, None, None)
    for args, msg in (((3, 1), "op 3"), ((_lib.FOCAL_MIN, 0), "radius 0 outside 1..15"), ((_lib.FOCAL_MAX, 16), "radius 16"),
                      ((_lib.FOCAL_MEDIAN, 4), "radius 4 outside 1..3"), ((_lib.FOCAL_MEDIAN, 1, 10), "min_count 10 outside 1..9")):
        with pytest.raises(InsarError, match="insar_focal_rank: .*" + msg):
            rank(*args)
    for h, msg in (((0.0, 1.0, 1.0, 1.0), "reciprocal spacing 0"), ((1.0, 1.0, float("inf"), 1.0), "reciprocal spacing inf")):
        with pytest.raises(InsarError, match="insar_focal_gradient: .*" + msg):
            _lib.call("insar_focal_gradient", a, 1, 4, 4, *h, 0, 0.0, None, 1, o, None, None)
    with pytest.raises(InsarError, match="insar_focal_gradient: nodata is NaN"):
        _lib.call("insar_focal_gradient", a, 1, 4, 4, 1.0, 0.5, 1.0, 0.5, 1, float("nan"), None, 1, o, None, None)


def test_detect_checks_smooth_before_predict_runs():
    kw = iu.ScenePredictor._contour_kwargs
    assert kw(dict(levels=[0.5], smooth=1.5))["smooth"] == 1.5 and kw(dict(levels=[0.5], smooth=5))["smooth"] == 5
    assert "smooth" not in kw(dict(levels=[0.5])) and kw(dict(levels=[0.5], smooth=None))["smooth"] is None
    for bad in (0, 0.0, -1.0, 5.01, float("nan"), float("inf"), "1.5", True, (1.5,)):
        with pytest.raises(InsarError, match="contours: smooth=.*0 < sigma <= 5"):
            kw(dict(levels=[0.5], smooth=bad))
