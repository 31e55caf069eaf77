"""Host: which tile shapes the per-tap implicit GEMM's selectors (insar_igemm_tile_rows / _tile_cols / _tile_cols_dt /
_num_mtiles, csrc/igemm.hip) can return with the knobs at their defaults, and the shapes tests/test_igemm_oob_exact_gpu.py
relies on. Host arithmetic only: runs without a GPU.

The sweep: M over every multiple of 128 up to 2^20 and its two neighbours (every boundary of a 128- or a 256-row tile), N over
{64, 128, 192, 256, 512, 1024, 2048}, both dtypes. It finds seven (rows, cols, dtype) combinations and NOT 128 x 128: with
bm = 128 and N % 128 == 0, igemm_bm_for has ceil(M / 256) * N / 64 < 128, hence ceil(M / 128) * N / 128 <= 128 <= 256 and
igemm_bn_for returns 64. So launch_igemm<.., 128, 128, 2> is unreachable in both dtypes under the default knobs."""
import pytest

from insar_unet_ca_amd import _lib

NS = (64, 128, 192, 256, 512, 1024, 2048)
REACHED = {(128, 64, "f32"), (128, 64, "bf16"), (256, 64, "f32"), (256, 64, "bf16"), (256, 128, "f32"), (256, 128, "bf16"),
           (256, 256, "bf16")}


def _ms():
    ms = {1}
    for m in range(128, (1 << 20) + 1, 128):
        ms.update((m - 1, m, m + 1))
    return sorted(m for m in ms if m <= 1 << 20)


def test_the_tile_shapes_the_selectors_can_return():
    call = _lib.call
    for knob in ("igemm_xwide_min", "igemm_wide_min"):
        assert _lib.tune(knob) == 0, f"{knob} is set: the sweep describes the default path"
    seen = set()
    for M in _ms():
        for N in NS:
            rows, cols = call("insar_igemm_tile_rows", M, N), call("insar_igemm_tile_cols", M, N)
            assert rows in (128, 256) and call("insar_igemm_num_mtiles", M, N) == -(-M // rows)
            f32, bf16 = call("insar_igemm_tile_cols_dt", M, N, _lib.F32), call("insar_igemm_tile_cols_dt", M, N, _lib.BF16)
            assert f32 == cols and bf16 in (cols, 256) and N % f32 == 0 and N % bf16 == 0
            assert bf16 != 256 or (rows == 256 and -(-M // 256) * (N // 256) >= 256)
            if rows == 128:                                     # the argument of the module docstring
                assert -(-M // 256) * (N // 64) < 128 and cols == 64
            seen.update(((rows, f32, "f32"), (rows, bf16, "bf16")))
    assert seen == REACHED
    assert (128, 128, "f32") not in seen and (128, 128, "bf16") not in seen


@pytest.mark.parametrize("wide,shape,bf16_tile,f32_tile", [
    (128, (2, 32, 32), (128, 64), (128, 64)), (128, (2, 16, 64), (128, 64), (128, 64)), (128, (3, 9, 13), (128, 64), (128, 64)),
    (512, (4, 32, 32), (256, 64), (256, 64)), (512, (5, 30, 30), (256, 64), (256, 64)),
    (512, (16, 32, 32), (256, 128), (256, 128)), (512, (17, 30, 34), (256, 128), (256, 128)),
    (2048, (8, 32, 32), (256, 256), (256, 128)), (2048, (9, 30, 30), (256, 256), (256, 128)),
    (64, (32, 32, 32), (256, 64), (256, 64)), (64, (3, 30, 34), (128, 64), (128, 64))])
def test_the_shapes_of_the_out_of_bounds_cases(wide, shape, bf16_tile, f32_tile):
    """The smallest shapes that reach each tile (tests/test_igemm_oob_exact_gpu.py asserts them again where it launches); the
    narrow side of each, N = 64, stays on 128 x 64 tiles except where the shape was chosen for 256 rows at N = 64."""
    call = _lib.call
    M = shape[0] * shape[1] * shape[2]
    rows = call("insar_igemm_tile_rows", M, wide)
    assert (rows, call("insar_igemm_tile_cols_dt", M, wide, _lib.BF16)) == bf16_tile
    assert (rows, call("insar_igemm_tile_cols_dt", M, wide, _lib.F32)) == f32_tile
    if wide != 64:
        assert call("insar_igemm_tile_rows", M, 64) == 128
