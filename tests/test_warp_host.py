"""CPU-only: the numpy restatement of csrc/warp.hip (tests/warp_ref.py) against cases that can be derived by hand, the host
side of insar_unet_ca_amd/warp.py (quantisation, grid_matrix, WarpSpec, every refusal that needs no device) and the ABI."""
import os

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _lib, warp
from insar_unet_ca_amd._lib import InsarError
from tests import warp_ref as ref

IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
NEW_NAMES = ["warp_raster", "grid_matrix", "multilook", "WarpSpec", "draw_warps", "gather_warped"]
NEW_SYMBOLS = ["insar_warp_raster", "insar_warp_gather", "insar_warp_draw", "insar_multilook"]


def _src(dtype, shape=(13, 17), seed=3):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        a = rng.standard_normal(shape).astype(np.float32)
        return a
    return rng.integers(0, 256, size=shape).astype(dtype)


def _same(a: np.ndarray, b: np.ndarray) -> bool:
    if a.dtype == np.float32:
        return b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- the reference against hand-derivable cases ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, mode", [(np.uint8, "nearest"), (np.uint8, "bilinear"), (np.float32, "nearest"),
                                         (np.float32, "bilinear"), (np.int32, "nearest")])
def test_identity_returns_the_source(dtype, mode):
    src = _src(dtype)
    out, valid = ref.warp(src, ref.quantise(IDENTITY), *src.shape, mode, 0)
    assert _same(out, src) and valid.all()
    planes = np.stack([src, src[::-1].copy()])
    out, _ = ref.warp(planes, ref.quantise(IDENTITY), *src.shape, mode, 0)
    assert _same(out, planes)


def test_quantised_identity_and_the_inside_rule():
    q = ref.quantise(IDENTITY)
    assert q.tolist() == [1 << 32, 0, 0, 0, 1 << 32, 0]
    sx, sy = ref.positions(q, 2, 3)
    assert sx.tolist() == [[0, 256, 512]] * 2 and sy.tolist() == [[0, 0, 0], [256, 256, 256]]
    # a pixel is inside iff its centre lies on [-0.5, W - 0.5): half a pixel to the left is in, half a pixel to the right is out
    src = np.arange(6, dtype=np.uint8).reshape(2, 3)
    _, valid = ref.warp(src, ref.quantise([[1, 0, -0.5], [0, 1, 0]]), 2, 4, "nearest", 9)
    assert valid.tolist() == [[1, 1, 1, 0]] * 2
    out, valid = ref.warp(src, ref.quantise([[1, 0, 0.5], [0, 1, 0]]), 2, 4, "nearest", 9)
    assert valid.tolist() == [[1, 1, 0, 0]] * 2 and out.tolist() == [[1, 2, 9, 9], [4, 5, 9, 9]]      # ties round up


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_quarter_turn_from_the_table_is_rot90(dtype, mode):
    table = ref.angle_table()
    assert table[0].tolist() == [1 << 30, 0] and table[256].tolist() == [0, 1 << 30]
    assert table[512].tolist() == [-(1 << 30), 0] and table[768].tolist() == [0, -(1 << 30)]
    N = 12
    src = _src(dtype, (N, N))
    for turns in (1, 2, 3):
        q = ref.tile_matrix((0, 0), N, 256 * turns, 256, table)
        out, valid = ref.warp(src, q, N, N, mode, 0)
        assert valid.all() and _same(out, np.ascontiguousarray(np.rot90(src, turns)))
    assert ref.tile_matrix((5, 9), N, 0, 256, table).tolist() == [1 << 32, 0, 9 << 32, 0, 1 << 32, 5 << 32]
    assert ref.tile_matrix((5, 9), N, -256, 256, table).tolist() == ref.tile_matrix((5, 9), N, 768, 256, table).tolist()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_integer_zoom_nearest_is_repeat(k):
    src = _src(np.int32, (7, 9))
    s = 1.0 / k                                              # index x of the fine grid has its centre at (x + 0.5) / k - 0.5
    q = ref.quantise([[s, 0, 0.5 * s - 0.5], [0, s, 0.5 * s - 0.5]])
    out, valid = ref.warp(src, q, 7 * k, 9 * k, "nearest", -1)
    assert valid.all() and _same(out, np.repeat(np.repeat(src, k, axis=0), k, axis=1))


@pytest.mark.parametrize("fy, fx", [(1, 1), (2, 2), (3, 5), (16, 16)])
def test_multilook_u8_is_the_rounded_mean(fy, fx):
    src = _src(np.uint8, (50, 83))
    h, w = 50 // fy, 83 // fx
    want = np.floor(src[:h * fy, :w * fx].reshape(h, fy, w, fx).astype(np.float64).mean(axis=(1, 3)) + 0.5).astype(np.uint8)
    got, count = ref.multilook(src, fy, fx)
    assert _same(got, want) and (count == fy * fx).all()


def test_multilook_f32_skips_nan():
    src = np.array([[1.0, np.nan, 2.0, 4.0], [3.0, 5.0, np.nan, np.nan]], dtype=np.float32)
    got, count = ref.multilook(src, 2, 2)
    assert got.tolist() == [[3.0, 3.0]] and count.tolist() == [[3, 2]]
    got, _ = ref.multilook(src, 2, 2, min_valid=3)
    assert got[0, 0] == 3.0 and np.isnan(got[0, 1])
    got, count = ref.multilook(np.full((2, 2), np.nan, dtype=np.float32), 2, 2)
    assert np.isnan(got[0, 0]) and count[0, 0] == 0


def test_bilinear_halfway_values():
    src = np.array([[0, 100], [200, 255]], dtype=np.uint8)
    q = ref.quantise([[1, 0, 0.5], [0, 1, 0.5]])
    assert ref.warp(src, q, 1, 1, "bilinear", 0)[0].tolist() == [[139]]            # 138.75 rounds to 139
    f = src.astype(np.float32)
    assert ref.warp(f, q, 1, 1, "bilinear", 0)[0].tolist() == [[138.75]]
    f[0, 1] = np.nan
    assert np.isnan(ref.warp(f, ref.quantise(IDENTITY), 2, 2, "bilinear", 0)[0][0]).all()    # a NaN tap gives NaN at weight 0 too


def test_draw_is_a_function_of_key_and_row():
    table = ref.angle_table()
    origins = np.array([[0, 0], [8, 24], [40, 16]], dtype=np.int32)
    same = ref.draw(77, origins, 16, 0, 256, 256, table)
    assert same.tolist() == [[1 << 32, 0, int(x) << 32, 0, 1 << 32, int(y) << 32] for y, x in origins]
    a, b = ref.draw(77, origins, 16, 40, 200, 400, table), ref.draw(78, origins, 16, 40, 200, 400, table)
    assert np.array_equal(a, ref.draw(77, origins, 16, 40, 200, 400, table)) and not np.array_equal(a, b)
    # the tile centre, index origin + (T - 1) / 2, stays where it is: twice the centre keeps the sums in integers
    for (y0, x0), m in zip(origins, a):
        m = [int(v) for v in m]
        assert abs(m[0] * 15 + m[1] * 15 + 2 * m[2] - ((2 * int(x0) + 15) << 32)) <= 1
        assert abs(m[3] * 15 + m[4] * 15 + 2 * m[5] - ((2 * int(y0) + 15) << 32)) <= 1


# ---- the host side of warp.py -----------------------------------------------------------------------------------------------
def test_quantise_matrix_bounds_and_refusals():
    assert np.array_equal(warp.quantise_matrix(IDENTITY), ref.quantise(IDENTITY))
    m = [[0.3, -1.7, 1048576.0], [2.5, 1e-9, -1048576.0]]
    assert np.array_equal(warp.quantise_matrix(m), ref.quantise(m)) and warp.quantise_matrix(m).dtype == np.int64
    assert warp.quantise_matrix(m)[2] == 1 << 52
    for bad in ([[1, 0, 1048577.0], [0, 1, 0]], [[1, 0, 0], [0, -1048576.5, 0]], [[np.nan, 0, 0], [0, 1, 0]],
                [[1, 0, 0], [0, np.inf, 0]], [[1, 0, 0]], np.eye(3), "matrix", None):
        with pytest.raises(InsarError):
            warp.quantise_matrix(bad)
    warp.check_extent(warp.quantise_matrix(m), 32768, 32768)
    with pytest.raises(InsarError, match="int64"):
        warp.check_extent(np.array([1 << 52, 1 << 52, 0, 0, 0, 0], dtype=np.int64), 32768, 32768)
    assert np.array_equal(warp.angle_table(), ref.angle_table()) and warp.WARP_STREAM == ref.WARP_STREAM


def test_grid_matrix_round_trip_and_convention():
    A = np.array([[30.0, 2.0, 500000.0], [-1.5, -30.0, 4100000.0]])
    B = np.array([[10.0, 0.0, 500123.0], [0.0, -10.0, 4099877.0]])
    ab, ba = iu.grid_matrix(A, B), iu.grid_matrix(B, A)
    full = lambda m: np.vstack([m, [0.0, 0.0, 1.0]])
    assert np.abs(full(ab) @ full(ba) - np.eye(3)).max() <= 1e-12
    assert np.abs(full(ba) @ full(ab) - np.eye(3)).max() <= 1e-12
    assert np.abs(iu.grid_matrix(A, A) - np.array(IDENTITY)).max() <= 1e-12
    # a grid of half the spacing with the same corner: fine index x has its centre at (x + 0.5) / 2 - 0.5 of the coarse grid
    coarse, fine = [[2.0, 0, 10.0], [0, -2.0, 50.0]], [[1.0, 0, 10.0], [0, -1.0, 50.0]]
    assert np.allclose(iu.grid_matrix(coarse, fine), [[0.5, 0, -0.25], [0, 0.5, -0.25]], atol=1e-15)
    # the pixel whose centre is the world point p in the destination grid maps to the pixel position of p in the source grid
    p = full(B) @ np.array([7.5, 3.5, 1.0])                       # centre of destination pixel (x, y) = (7, 3)
    want = np.linalg.solve(full(A), p)[:2] - 0.5
    assert np.abs(ab @ np.array([7.0, 3.0, 1.0]) - want).max() <= 1e-9
    for bad in ([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]], [[np.nan, 0, 0], [0, 1, 0]], [[1.0, 0.0], [0.0, 1.0]]):
        with pytest.raises(InsarError):
            iu.grid_matrix(bad, B)
        with pytest.raises(InsarError):
            iu.grid_matrix(A, bad)


def test_warp_spec():
    s = iu.WarpSpec()
    assert s.config() == {"zoom_q8": [256, 256], "amax": 0}
    s = iu.WarpSpec(zoom=(0.75, 1.3), max_angle_deg=45)
    assert s.config() == {"zoom_q8": [192, 333], "amax": 128}
    assert iu.WarpSpec(max_angle_deg=180).amax == 512
    for kw in ({"zoom": (0, 1)}, {"zoom": (1.2, 1.0)}, {"zoom": (1, 17)}, {"zoom": 1.0}, {"zoom": (1, np.nan)},
               {"max_angle_deg": -1}, {"max_angle_deg": 181}, {"max_angle_deg": "x"}, {"zoom": (0.001, 1)}):
        with pytest.raises(InsarError):
            iu.WarpSpec(**kw)


def test_cpu_tensors_and_bad_objects_are_refused():
    src = torch.zeros(8, 8)
    with pytest.raises(InsarError, match="ROCm"):
        iu.warp_raster(src, IDENTITY, (8, 8))
    with pytest.raises(InsarError, match="ROCm"):
        iu.warp_raster(np.zeros((8, 8), dtype=np.float32), IDENTITY, (8, 8))
    with pytest.raises(InsarError, match="ROCm"):
        iu.multilook(src, 2)
    with pytest.raises(InsarError, match="ROCm"):
        iu.draw_warps(1, torch.zeros(2, 2, dtype=torch.int32), 16, iu.WarpSpec())
    with pytest.raises(InsarError, match="WarpSpec"):
        iu.draw_warps(1, torch.zeros(2, 2, dtype=torch.int32), 16, None)
    with pytest.raises(InsarError, match="ROCm"):
        iu.gather_warped(torch.zeros(8, 8), None, torch.zeros(1, 6, dtype=torch.int64), 8)
    with pytest.raises(InsarError, match="neither"):
        iu.gather_warped(None, None, torch.zeros(1, 6, dtype=torch.int64), 8)
    scene, labels = np.zeros((32, 32), dtype=np.uint8), np.zeros((32, 32), dtype=np.uint8)
    with pytest.raises(InsarError, match="WarpSpec"):
        iu.SceneCrops(scene, labels, tile=16, batch=2, warp=(1.0, 1.0))


def test_entry_points_refuse_before_the_device():
    """Every entry point validates its arguments before it touches the device: the error paths run without one."""
    call, P = _lib.call, 4096                                                   # P: an aligned pointer that is never followed
    R = lambda *a: call("insar_warp_raster", *a)
    ok = dict(src=P, dtype=_lib.WARP_F32, C=1, H=8, W=8, mats=P, n=1, h=8, w=8, mode=_lib.WARP_BILINEAR, fill=0, dst=P, valid=None)
    for change, pattern in (({"src": None}, "null"), ({"mats": None}, "null"), ({"dst": None}, "null"), ({"dtype": 3}, "dtype"),
                            ({"mode": 2}, "mode"), ({"dtype": _lib.WARP_I32}, "bilinear on int32"), ({"C": 5}, "channels"),
                            ({"C": 0}, "channels"), ({"H": 0}, "empty"), ({"H": 65536, "W": 32768}, "2\\^31"), ({"n": 0}, "n = 0"),
                            ({"h": 0}, "output"), ({"w": 32769}, "output"), ({"src": P + 2}, "aligned"), ({"mats": P + 4}, "8-byte")):
        a = dict(ok, **change)
        with pytest.raises(InsarError, match=pattern):
            R(a["src"], a["dtype"], a["C"], a["H"], a["W"], a["mats"], a["n"], a["h"], a["w"], a["mode"], a["fill"], a["dst"], a["valid"], None)
    G = lambda *a: call("insar_warp_gather", *a)
    U8, I64 = _lib.AUG_MASK_U8, _lib.AUG_MASK_I64
    for args, pattern in (((P, 0, P, 8, 8, None, 1, 8, 0.0, P, P, I64), "null"), ((P, 0, P, 8, 8, P, 1, 8, 0.0, None, None, I64), "neither"),
                          ((None, 0, P, 8, 8, P, 1, 8, 0.0, P, P, I64), "scene"), ((P, 0, None, 8, 8, P, 1, 8, 0.0, P, P, I64), "labels"),
                          ((P, 2, P, 8, 8, P, 1, 8, 0.0, P, P, I64), "scene dtype"), ((P, 0, P, 8, 8, P, 1, 8, 0.0, P, P, 0), "mask dtype"),
                          ((P, 0, P, 8, 8, P, 1, 6, 0.0, P, P, I64), "multiple of 4"), ((P, 0, P, 8, 8, P, 0, 8, 0.0, P, P, I64), "n = 0"),
                          ((P, 0, P, 8, 8, P, 1, 8, 0.0, P + 4, P, I64), "16-byte"), ((P, 0, P, 8, 8, P, 1, 8, 0.0, P, P + 8, I64), "masks not aligned"),
                          ((P, 0, P, 8, 8, P, 1, 8, 0.0, P, P + 2, U8), "masks not aligned")):
        with pytest.raises(InsarError, match=pattern):
            G(*args, None)
    D = lambda *a: call("insar_warp_draw", *a)
    for args, pattern in (((1, None, 1, 16, 0, 256, 256, P, P), "null"), ((1, P, 0, 16, 0, 256, 256, P, P), "n = 0"),
                          ((1, P, 1, 0, 0, 256, 256, P, P), "tile"), ((1, P, 1, 16, 513, 256, 256, P, P), "amax"),
                          ((1, P, 1, 16, -1, 256, 256, P, P), "amax"), ((1, P, 1, 16, 0, 0, 256, P, P), "zoom"),
                          ((1, P, 1, 16, 0, 300, 256, P, P), "zoom"), ((1, P, 1, 16, 0, 256, 4097, P, P), "zoom"),
                          ((1, P, 1, 16, 0, 256, 256, P, P + 4), "8-byte")):
        with pytest.raises(InsarError, match=pattern):
            D(*args, None)
    M = lambda *a: call("insar_multilook", *a)
    F, B = _lib.WARP_F32, _lib.WARP_U8
    for args, pattern in (((None, F, 1, 8, 8, 2, 2, 1, P, None), "null"), ((P, _lib.WARP_I32, 1, 8, 8, 2, 2, 1, P, None), "dtype"),
                          ((P, F, 1, 8, 8, 0, 2, 1, P, None), "factors"), ((P, F, 1, 8, 8, 2, 17, 1, P, None), "factors"),
                          ((P, B, 1, 8, 20, 9, 2, 1, P, None), "above the source"), ((P, F, 1, 8, 8, 2, 2, 0, P, None), "min_valid"),
                          ((P, F, 1, 8, 8, 2, 2, 5, P, None), "min_valid"), ((P, F, 5, 8, 8, 2, 2, 1, P, None), "channels"),
                          ((P, F, 1, 8, 8, 2, 2, 1, P + 1, None), "aligned"), ((P, F, 1, 8, 8, 2, 2, 1, P, P + 2), "count")):
        with pytest.raises(InsarError, match=pattern):
            M(*args, None)


def test_exports_and_abi():
    assert _lib.ABI_VERSION == 8 and _lib.load().insar_version() == 8
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "insar_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header
    for name in NEW_NAMES:
        assert name in iu.__all__ and hasattr(iu, name)
    assert (_lib.WARP_U8, _lib.WARP_I32, _lib.WARP_F32, _lib.WARP_NEAREST, _lib.WARP_BILINEAR) == (0, 1, 2, 0, 1)
