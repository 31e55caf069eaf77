"""Host-only: the numpy restatement of tests/zonal_ref.py pinned against a brute-force per-region loop, the argument checks
of insar_unet_ca_amd/zonal.py (all of which come before the device is touched), the table arithmetic, the bindings, the
percentile rule and the host formation of the float fields from the raw integers."""
import ctypes
import math
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from insar_unet_ca_amd import _lib, zonal
from insar_unet_ca_amd._lib import InsarError
from tests import zonal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("insar_zonal_scratch_bytes", "insar_zonal_clear", "insar_zonal_accumulate")


# ---- the restatement against a pixel loop ---------------------------------------------------------------------------------
def brute_force(labels, raster, max_regions, scale, nodata, bins, rng_q):
    """One pass over the pixels in row-major order with Python ints; ties keep the first pixel."""
    H, W = labels.shape
    regs = {}
    oor = 0
    for y in range(H):
        for x in range(W):
            l = int(labels[y, x])
            if l > max_regions:
                oor += 1
            if l < 1 or l > max_regions:
                continue
            r = regs.setdefault(l, dict(n=0, n_invalid=0, n_clipped=0, sum_q=0, sumsq_q=0, min_q=None, max_q=None, argmin=None,
                                        argmax=None, hist=[0] * bins, below=0, above=0, values=[]))
            v = raster[y, x]
            if raster.dtype == np.float32:
                if not math.isfinite(float(v)) or (nodata is not None and v == np.float32(nodata)):
                    r["n_invalid"] += 1
                    continue
                d = float(v) * float(scale)                       # float32 -> float64 is exact, then one float64 product
                if abs(d) > ref.Q_LIMIT:
                    r["n_clipped"] += 1
                    d = math.copysign(float(ref.Q_LIMIT), d)
                q = round(d)                                      # Python rounds halves to even
            else:
                if nodata is not None and int(v) == int(nodata):
                    r["n_invalid"] += 1
                    continue
                q = int(v)
            r["n"] += 1
            r["sum_q"] += q
            r["sumsq_q"] += q * q
            r["values"].append(q)
            if r["min_q"] is None or q < r["min_q"]:
                r["min_q"], r["argmin"] = q, (y, x)
            if r["max_q"] is None or q > r["max_q"]:
                r["max_q"], r["argmax"] = q, (y, x)
            if bins:
                lo, hi = rng_q
                if q < lo:
                    r["below"] += 1
                elif q >= hi:
                    r["above"] += 1
                else:
                    r["hist"][(q - lo) * bins // (hi - lo)] += 1
    return regs, oor


def _small_map(seed, H, W, nlab, dtype):
    rng = np.random.default_rng(seed)
    labels = rng.integers(-1, nlab + 3, size=(H, W)).astype(np.int32)
    labels[labels == 2] = 0                                       # id 2 is unused
    if dtype == np.float32:
        raster = (rng.normal(size=(H, W)) * 3).astype(np.float32)
        raster.ravel()[rng.integers(0, H * W, size=12)] = [np.nan, np.inf, -np.inf, -0.0, 7.5, 7.5, 1e6, -1e6, 0.5 / 65536,
                                                           1.5 / 65536, 2.5 / 65536, -0.5 / 65536]
    elif dtype == np.uint8:
        raster = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    else:
        raster = rng.integers(-1000, 1000, size=(H, W)).astype(np.int32)
        raster[0, :2] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    return labels, raster


@pytest.mark.parametrize("dtype,nodata,bins,rng", [(np.float32, 7.5, 0, None), (np.float32, None, 7, (-4.0, 4.0)),
                                                   (np.uint8, 3, 5, (10, 200)), (np.int32, None, 4, (-500, 500))])
def test_restatement_equals_a_pixel_loop(dtype, nodata, bins, rng):
    labels, raster = _small_map(7, 23, 31, 9, dtype)
    R = 10                                                        # labels 11 occur and are out of range
    got = ref.region_stats_ref(labels, raster, max_regions=R, nodata=nodata, bins=bins, range=rng)
    scale = 65536.0 if dtype == np.float32 else 1.0
    regs, oor = brute_force(labels, raster, R, 65536.0, nodata, bins, got["range_q"])
    assert got["out_of_range"] == oor > 0
    assert got["n"][1] == 0 and got["n_invalid"][1] == 0 and np.isnan(got["mean"][1]) and tuple(got["argmin"][1]) == (-1, -1)
    for l in range(1, R + 1):
        r = regs.get(l)
        if r is None:
            assert got["n"][l - 1] == 0 and got["n_invalid"][l - 1] == 0
            continue
        for f in ("n", "n_invalid", "n_clipped", "sum_q", "sumsq_q"):
            assert int(got[f][l - 1]) == r[f], (l, f)
        if r["n"] == 0:
            continue
        assert int(got["min_q"][l - 1]) == r["min_q"] and int(got["max_q"][l - 1]) == r["max_q"]
        assert tuple(got["argmin"][l - 1]) == r["argmin"] and tuple(got["argmax"][l - 1]) == r["argmax"], l
        if bins:
            assert got["hist"][l - 1].tolist() == r["hist"] and got["below"][l - 1] == r["below"] and got["above"][l - 1] == r["above"]
            assert sum(r["hist"]) + r["below"] + r["above"] == r["n"]
        mean = math.fsum(r["values"]) / r["n"]
        var = Fraction(r["n"] * r["sumsq_q"] - r["sum_q"] ** 2, r["n"] ** 2)
        np.testing.assert_allclose(got["mean"][l - 1], mean / scale, rtol=1e-12)
        np.testing.assert_allclose(got["std"][l - 1], math.sqrt(var) / scale, rtol=1e-12)
        np.testing.assert_allclose(got["sum"][l - 1], math.fsum(r["values"]) / scale, rtol=1e-12)
        assert got["min"][l - 1] == r["min_q"] / scale and got["max"][l - 1] == r["max_q"] / scale
    if dtype == np.float32:
        assert got["n_clipped"].sum() == 2 and got["n_invalid"].sum() >= 1


def test_quantisation_rounds_halves_to_even_and_clamps():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3e9, -3e9, 2147483520.0, -0.0], dtype=np.float32)
    q, valid, clipped = ref.quantise(v, 1.0)
    assert q.tolist() == [0, 2, 2, 0, -2, ref.Q_LIMIT, -ref.Q_LIMIT, 2147483520, 0]
    assert valid.all() and clipped.tolist() == [False] * 5 + [True, True, False, False]
    assert zonal.quantise_scalar(2.5, 1.0) == 2 and zonal.quantise_scalar(-1e300, 1e300) == -ref.Q_LIMIT
    assert ref.quantise_scalar(0.25, 65536.0) == zonal.quantise_scalar(0.25, 65536.0) == 16384


# ---- argument checks: before anything touches the device ------------------------------------------------------------------
def _ok():
    return torch.zeros(6, 8, dtype=torch.int32), torch.zeros(6, 8, dtype=torch.float32)


def test_a_cpu_tensor_is_refused():
    labels, raster = _ok()
    with pytest.raises(InsarError, match="ROCm"):
        zonal.region_stats(labels, raster)
    with pytest.raises(InsarError, match="torch tensors"):
        zonal.region_stats(labels.numpy(), raster)


@pytest.mark.parametrize("make,kw,match", [
    (lambda l, r: (l.long(), r), {}, "int32"),
    (lambda l, r: (l[None], r), {}, "2-D"),
    (lambda l, r: (l, r.double()), {}, "dtype"),
    (lambda l, r: (l, r[:, :7]), {}, r"\[6, 8\]"),
    (lambda l, r: (l, r[None, None]), {}, r"\[6, 8\]"),
    (lambda l, r: (l, torch.zeros(5, 6, 8)), {}, "channels"),
    (lambda l, r: (torch.zeros(6, 16, dtype=torch.int32)[:, ::2], r), {}, "contiguous"),
    (lambda l, r: (l, torch.zeros(8, 6).t()), {}, "contiguous"),
    (lambda l, r: (l, r), {"bins": -1}, "bins"),
    (lambda l, r: (l, r), {"bins": 257, "range": (0, 1)}, "bins"),
    (lambda l, r: (l, r), {"bins": 2.5, "range": (0, 1)}, "bins"),
    (lambda l, r: (l, r), {"bins": 4}, "range"),
    (lambda l, r: (l, r), {"bins": 4, "range": (0.0, math.inf)}, "range"),
    (lambda l, r: (l, r), {"bins": 4, "range": (math.nan, 1.0)}, "range"),
    (lambda l, r: (l, r), {"bins": 4, "range": (1.0, 1.0)}, "lo >= hi"),
    (lambda l, r: (l, r), {"bins": 4, "range": (0.0, 1e-9)}, "lo >= hi"),          # equal after quantisation
    (lambda l, r: (l, r), {"bins": 4, "range": (2.0, 1.0)}, "lo >= hi"),
    (lambda l, r: (l, r), {"scale": 0.0}, "scale"),
    (lambda l, r: (l, r), {"scale": -1.0}, "scale"),
    (lambda l, r: (l, r), {"scale": math.inf}, "scale"),
    (lambda l, r: (l, r), {"scale": math.nan}, "scale"),
    (lambda l, r: (l, r), {"nodata": math.nan}, "NaN"),
    (lambda l, r: (l, r.to(torch.uint8)), {"nodata": 256}, "nodata"),
    (lambda l, r: (l, r.to(torch.int32)), {"nodata": 0.5}, "nodata"),
    (lambda l, r: (l, r), {"max_regions": 0}, "max_regions"),
    (lambda l, r: (l, r), {"max_regions": 4, "count": 5}, "count"),
])
def test_argument_checks_raise_on_the_host(make, kw, match):
    labels, raster = make(*_ok())
    with pytest.raises(InsarError, match=match):
        zonal.region_stats(labels, raster, **kw)


def test_a_scratch_of_the_wrong_size_is_refused():
    labels, raster = _ok()
    stub = lambda R, b, c, nbytes: types.SimpleNamespace(max_regions=R, bins=b, channels=c, table=torch.zeros(nbytes, dtype=torch.uint8))
    want = zonal.scratch_bytes(16, 0, 1)
    for sc in (stub(8, 0, 1, zonal.scratch_bytes(8, 0, 1)), stub(16, 4, 1, zonal.scratch_bytes(16, 4, 1)),
               stub(16, 0, 2, zonal.scratch_bytes(16, 0, 2)), stub(16, 0, 1, want - 16)):
        with pytest.raises(InsarError, match="scratch"):
            zonal.region_stats(labels, raster, max_regions=16, scratch=sc)
    with pytest.raises(InsarError, match="ROCm"):                 # the right size passes this check and meets the last one
        zonal.region_stats(labels, raster, max_regions=16, scratch=stub(16, 0, 1, want))


def test_entry_points_refuse_before_the_device():
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_zonal_clear", None, 4, 0, 1, None)
    with pytest.raises(InsarError, match="aligned"):
        _lib.call("insar_zonal_clear", p + 4, 4, 0, 1, None)
    acc = lambda **o: _lib.call("insar_zonal_accumulate", *[{**dict(labels=p, raster=p, et=_lib.ZONAL_F32, C=1, H=4, W=4, scale=1.0,
                                                                     hn=0, nd=0.0, bins=0, lo=0, hi=0, R=4, table=p, s=None), **o}[k]
                                                            for k in ("labels", "raster", "et", "C", "H", "W", "scale", "hn", "nd", "bins",
                                                                      "lo", "hi", "R", "table", "s")])
    for o, match in ((dict(labels=None), "null"), (dict(et=3), "element type"), (dict(C=5), "channels"), (dict(H=0), "empty"),
                     (dict(H=65536, W=65536), "2\\^31"), (dict(scale=0.0), "scale"), (dict(scale=math.inf), "scale"),
                     (dict(hn=1, nd=math.nan), "NaN"), (dict(bins=300), "bins"), (dict(bins=4, lo=5, hi=5), "range"),
                     (dict(R=0), "max_regions"), (dict(table=None), "null"), (dict(labels=p + 2), "aligned"),
                     (dict(et=_lib.ZONAL_I32, hn=1, nd=0.5), "nodata")):
        with pytest.raises(InsarError, match=match):
            acc(**o)


# ---- table arithmetic and bindings ----------------------------------------------------------------------------------------
def test_scratch_bytes_is_host_arithmetic_and_monotone():
    assert zonal.scratch_bytes(1, 0, 1) == 128
    assert zonal.scratch_bytes(65536, 0, 1) == 64 * 65537
    assert zonal.scratch_bytes(3, 7, 2) == 64 * 7 + ((4 * 2 * 3 * 7 + 15) // 16) * 16
    prev = 0
    for R in (1, 2, 100, 65536, 1 << 24):
        for bins in (0, 1, 7, 256):
            for ch in (1, 2, 4):
                b = zonal.scratch_bytes(R, bins, ch)
                assert b % 16 == 0
                assert b >= zonal.scratch_bytes(max(R - 1, 1), bins, ch) and b >= zonal.scratch_bytes(R, max(bins - 1, 0), ch)
                assert b >= zonal.scratch_bytes(R, bins, max(ch - 1, 1))
        assert zonal.scratch_bytes(R, 0, 1) > prev
        prev = zonal.scratch_bytes(R, 0, 1)
    for bad in ((0, 0, 1), ((1 << 24) + 1, 0, 1), (4, -1, 1), (4, 257, 1), (4, 0, 0), (4, 0, 5)):
        with pytest.raises(InsarError):
            zonal.scratch_bytes(*bad)


def test_symbols_are_declared_exported_and_bound():
    assert _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert lib.insar_version() == 8
    header = open(os.path.join(ROOT, "include", "insar_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert len(_lib._SIGNATURES["insar_zonal_accumulate"]) == 15
    import insar_unet_ca_amd as iu
    assert iu.region_stats is zonal.region_stats and iu.ZonalScratch is zonal.ZonalScratch and iu.percentile is zonal.percentile


def test_record_layout_matches_the_c_compiler(tmp_path):
    import subprocess
    fields = [n for n in zonal.ZONAL_DTYPE.names]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "insar_hip.h")}"', "int main(void){",
           'printf("size %zu\\n", sizeof(InsarZonalStat));']
    src += [f'printf("{f} %zu\\n", offsetof(InsarZonalStat, {f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "z.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "z"), str(tmp_path / "z.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "z")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == zonal.ZONAL_DTYPE.itemsize == 64
    for f in fields:
        assert int(got[f]) == zonal.ZONAL_DTYPE.fields[f][1], f


# ---- host formation of the result -----------------------------------------------------------------------------------------
def _raw_table(records, max_regions, bins=0, hist=None, out_of_range=0):
    raw = np.zeros(zonal.scratch_bytes(max_regions, bins, 1), dtype=np.uint8)
    rec = raw[:64 * (1 + max_regions)].view(zonal.ZONAL_DTYPE)
    rec["min_key"][1:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    rec["sum_q"][0] = out_of_range
    for i, r in enumerate(records, start=1):
        for k, v in r.items():
            rec[k][i] = v
    if hist is not None:
        raw[64 * (1 + max_regions):64 * (1 + max_regions) + 4 * max_regions * bins].view("<u4")[:] = np.asarray(hist, dtype="<u4").ravel()
    return raw


def test_std_of_a_region_whose_square_sum_exceeds_64_bits():
    """n = 2^20 pixels, half at q = 2^31 - 1 and half at -(2^31 - 1): the square sum is 2^20 (2^31 - 1)^2 ~ 2^82, the sum 0,
    the population std exactly (2^31 - 1) / scale. Then the same with an offset, against exact rational arithmetic."""
    L, n = ref.Q_LIMIT, 1 << 20
    ss = n * L * L
    assert ss > 1 << 64
    lo_word, hi_word = n * ((L * L) & 0xFFFFFFFF), n * ((L * L) >> 32)
    assert lo_word + (hi_word << 32) == ss and lo_word < 1 << 63 and hi_word < 1 << 63
    key = lambda q, idx: ((q + (1 << 31)) << 32) | idx
    a, b = L, L - 12345
    n2 = 3
    ss2, s2 = a * a + 2 * b * b, a + 2 * b
    recs = [dict(n=n, sum_q=0, sumsq_lo=lo_word, sumsq_hi=hi_word, min_key=key(-L, 5), max_key=key(L, 0xFFFFFFFF & ~9)),
            dict(n=n2, sum_q=s2, sumsq_lo=ss2 & 0xFFFFFFFF, sumsq_hi=ss2 >> 32, min_key=key(b, 7), max_key=key(a, 0xFFFFFFFF & ~2)),
            dict(n_invalid=4)]
    st = zonal.stats_from_table(_raw_table(recs, 4, out_of_range=11), max_regions=4, channels=1, bins=0, count=3, shape=(3, 4),
                                scale=65536.0, is_float=True)
    assert st["sumsq_q"].dtype == object and st["sumsq_q"][0] == ss and st["sumsq_q"][1] == ss2 and st["out_of_range"] == 11
    assert st["std"][0] == L / 65536.0 and st["mean"][0] == 0.0
    exact = math.sqrt(Fraction(n2 * ss2 - s2 * s2, n2 * n2)) / 65536.0
    np.testing.assert_allclose(st["std"][1], exact, rtol=1e-12)
    # the naive float64 route loses it: the two terms agree to about 2^-36 of their size
    assert st["min_q"].tolist() == [-L, b, 0] and st["max_q"].tolist() == [L, a, 0]
    assert st["argmin"].tolist() == [[1, 1], [1, 3], [-1, -1]] and st["argmax"].tolist() == [[2, 1], [0, 2], [-1, -1]]
    assert st["n"].tolist() == [n, n2, 0] and st["n_invalid"].tolist() == [0, 0, 4]
    assert np.isnan(st["mean"][2]) and np.isnan(st["std"][2]) and np.isnan(st["min"][2]) and np.isnan(st["sum"][2])
    assert st["max"][1] == a / 65536.0 and st["sum"][1] == s2 / 65536.0
    assert st["argmin"].dtype == np.int32 and st["mean"].dtype == np.float64


def _hist_stats(hist, below, above, q_range, scale=1.0):
    hist = np.asarray(hist, dtype=np.int64)
    below, above = np.asarray(below, dtype=np.int64), np.asarray(above, dtype=np.int64)
    return {"hist": hist, "below": below, "above": above, "n": hist.sum(axis=-1) + below + above, "range_q": q_range, "scale": scale,
            "bins": hist.shape[-1]}


def test_percentile_on_hand_made_histograms():
    st = _hist_stats([[0, 10, 0, 10], [4, 0, 0, 0], [0, 0, 0, 0]], [0, 0, 0], [0, 0, 0], (0, 4))
    np.testing.assert_allclose(zonal.percentile(st, 50)[:2], [2.0, 0.5], rtol=1e-15)
    np.testing.assert_allclose(zonal.percentile(st, 25)[:2], [1.5, 0.25], rtol=1e-15)
    np.testing.assert_allclose(zonal.percentile(st, 75)[:2], [3.5, 0.75], rtol=1e-15)
    np.testing.assert_allclose(zonal.percentile(st, 0)[:2], [1.0, 0.0], rtol=1e-15)
    np.testing.assert_allclose(zonal.percentile(st, 100)[:2], [4.0, 1.0], rtol=1e-15)
    assert np.isnan(zonal.percentile(st, 50)[2])
    # pixels outside the range: inside `below` the lower end, beyond the last bin the upper end; raster units = q / scale
    st = _hist_stats([[10]], [5], [5], (0, 65536), scale=65536.0)
    np.testing.assert_allclose([zonal.percentile(st, p)[0] for p in (10, 25, 50, 75, 90)], [0.0, 0.0, 0.5, 1.0, 1.0], rtol=1e-15)
    # a [C, N, bins] stack gives [C, N]
    st = _hist_stats([[[2, 2]], [[4, 0]]], [[0], [0]], [[0], [0]], (-2, 2))
    np.testing.assert_allclose(zonal.percentile(st, 50), [[0.0], [-1.0]], rtol=1e-15, atol=0)
    with pytest.raises(InsarError, match="histogram"):
        zonal.percentile({"n": np.zeros(1)}, 50)
    with pytest.raises(InsarError, match="0..100"):
        zonal.percentile(st, 101)


def test_histogram_layout_of_the_host_table():
    hist = np.arange(2 * 3, dtype=np.uint32).reshape(2, 3)
    recs = [dict(n=3, below=1, above=2, min_key=1 << 63, max_key=(1 << 63) | 0xFFFFFFFF), dict(n=12, min_key=1 << 63, max_key=(1 << 63) | 0xFFFFFFFF)]
    st = zonal.stats_from_table(_raw_table(recs, 2, bins=3, hist=hist), max_regions=2, channels=1, bins=3, count=None, shape=(2, 2),
                                scale=1.0, is_float=False, q_range=(0, 3))
    assert st["hist"].tolist() == hist.tolist() and st["below"].tolist() == [1, 0] and st["above"].tolist() == [2, 0]
    assert st["range_q"] == (0, 3) and st["bins"] == 3 and st["min_q"].tolist() == [0, 0]
