"""GPU: the epilogue variants of the tiled convolution kernels (csrc/conv_epilogue.h) that tests/test_parity_gpu.py and
tests/test_bstat_gpu.py do not reach: BatchNorm partial sums carried over the tiles of a persistent 8-wave work-group (in
LDS slots and in registers), and the BatchNorm-backward sums of the consumer unit (InsarBstat) on row tiles (8-wave kernel,
its dilated form, the two-work-group kernel with one tile per group and with persistent groups).

Tolerances are the ones of those two files: the slab against float64 sums of the stored output 1e-4, the bstat slab
against the reduce pass 2e-5, and the float64 anchor of tests/test_bn_backward_chain_gpu.py."""
import ctypes as C

import pytest
import torch

from oracle import closed_form as cf
from tests.helpers import max_rel
from tests.test_bstat_gpu import _assert_float64_sums, _rand_act, _reference_sums
from tests.test_parity_gpu import _act_from, _halo_abs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def run_carried(dev, dtype, cout):
    """Forward 64 -> cout over 1 x 256 x 256 through the 8-wave flat kernel, persistent with ping-pong steps (flip 4 | 2) and
    one work-group per tile (flip 2). Returns (y, slab, rows the persistent launch writes, M tiles, y of the flip-2 launch)."""
    from insar_unet_ca_amd import _lib, engine
    from insar_unet_ca_amd._lib import call, ptr
    cin, h, w = 64, 256, 256
    ctx = engine.Ctx(dev, dtype)
    xa = _act_from(cf.make_input_random((1, cin, h, w), seed=5), dtype, dev)
    wf = engine.GemmWeight(ctx, torch.nn.Parameter(cf.fill_tensor("weight", (cout, cin, 3, 3), 11).to(dev)), "conv3").fwd()
    mtiles = call("insar_conv3x3_flat_num_mtiles", xa.ref)
    prow = call("insar_conv3x3_flat_stat_rows", xa.ref, cout, 4 | 2)
    ya, yb = (engine.Act.alloc(1, h, w, cout, dtype, dev) for _ in range(2))
    stats = torch.zeros(mtiles, 2, cout, device=dev)
    call("insar_conv3x3_flat", xa.ref, ya.ref, ptr(wf), 4 | 2, ptr(stats), _lib.stream_ptr())
    call("insar_conv3x3_flat", xa.ref, yb.ref, ptr(wf), 2, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    return ya, stats, prow, mtiles, yb


@pytest.mark.parametrize("dtype,cout", [(torch.bfloat16, 128), (torch.bfloat16, 64), (torch.float32, 128)],
                         ids=["bf16-128-lds-carry", "bf16-64-register-carry", "f32-128-register-carry"])
def test_flat_kernel_carried_sums(dev, dtype, cout):
    """263 tiles of 254 padded pixels: one more step than the 256 work-groups of a persistent grid, so every work-group
    carries its sums over at least one tile boundary and folds them once, into its own slab row."""
    ya, stats, prow, mtiles, yb = run_carried(dev, dtype, cout)
    assert mtiles == 263
    if not prow < mtiles:
        pytest.skip("this device runs the launch with one work-group per tile: nothing is carried")
    assert float(stats[prow:].abs().max()) == 0.0
    got = ya.nchw().double().cpu()
    assert float(got.abs().max()) > 0
    assert max_rel(stats.sum(0)[0], got.sum((0, 2, 3))) <= 1e-4
    assert max_rel(stats.sum(0)[1], (got ** 2).sum((0, 2, 3))) <= 1e-4
    assert torch.equal(ya.buf, yb.buf)
    assert _halo_abs(ya) == 0.0


def run_rows_bstat(dev, flags, shape, cin, cout, dtype=torch.bfloat16):
    """Input gradient of a cin -> cout conv over shape = (B, H, W) on row tiles with the consumer's BatchNorm-backward sums
    in the slab, and the same launch without them. Returns (dx, slab, y, scale, shift, dx of the plain launch)."""
    from insar_unet_ca_amd import _lib, engine
    from insar_unet_ca_amd._lib import call, ptr
    B, H, W = shape
    ctx = engine.Ctx(dev, dtype)
    dy = _rand_act(B, H, W, cout, dtype, dev, 5)
    y = _rand_act(B, H, W, cin, dtype, dev, 6)
    dx, dx2 = (engine.Act.alloc(B, H, W, cin, dtype, dev) for _ in range(2))
    wd = engine.GemmWeight(ctx, torch.nn.Parameter(torch.randn(cout, cin, 3, 3, device=dev) * 0.05), "conv3").dgrad()
    scale, shift = torch.randn(cin, device=dev), torch.randn(cin, device=dev) * 0.3
    slab = torch.zeros(call("insar_conv3x3_flat_stat_rows", dy.ref, cin, flags), 2, cin, device=dev)
    bs = _lib.InsarBstat(y.buf.data_ptr(), ptr(scale), ptr(shift))
    call("insar_conv3x3_flat_bstat", dy.ref, dx.ref, ptr(wd), flags, ptr(slab), C.byref(bs), _lib.stream_ptr())
    call("insar_conv3x3_flat", dy.ref, dx2.ref, ptr(wd), flags, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    return dx, slab, y, scale, shift, dx2


ROWS_BSTAT_CASES = [
    # the 8-wave kernel's row tiles
    (1 | 8 | 2, (2, 16, 32), 64, 128), (1 | 8 | 2, (2, 16, 32), 128, 64),
    (1 | 8 | 2, (3, 4, 128), 64, 128), (1 | 8 | 2, (3, 4, 128), 128, 64),
    # ... dilated by 2
    (1 | 8 | 2 | (2 << 8), (2, 16, 32), 64, 64),
    # the two-work-group kernel's row tiles, one tile per work-group
    (1 | 32 | 8, (2, 16, 32), 64, 128), (1 | 32 | 8, (2, 16, 32), 128, 64),
    (1 | 32 | 8, (3, 4, 128), 64, 128), (1 | 32 | 8, (3, 4, 128), 128, 64),
    # ... persistent: 640 tiles. 64 output columns: three work-groups per CU, the sums are carried where that is fewer than 640
    # (not on 256 CUs); 128 output columns: two per CU, 512 on 256 CUs, the sums are carried
    (1 | 32 | 8 | 4, (10, 128, 128), 64, 64), (1 | 32 | 8 | 4, (10, 128, 128), 128, 64),
]


@pytest.mark.parametrize("flags,shape,cin,cout", ROWS_BSTAT_CASES)
def test_row_tiles_bstat_sums(dev, flags, shape, cin, cout):
    dx, slab, y, scale, shift, dx2 = run_rows_bstat(dev, flags, shape, cin, cout)
    ref_tot, _ = _reference_sums(dx, y, scale, shift, dev)
    den = ref_tot.abs().max().item()
    assert den > 0
    assert (slab.double().sum(0) - ref_tot).abs().max().item() <= 2e-5 * den
    _assert_float64_sums(slab, dx, y, scale, shift)
    assert torch.equal(dx.buf, dx2.buf)
