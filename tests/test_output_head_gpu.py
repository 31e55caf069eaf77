"""GPU: the 1x1 output head (csrc/direct.hip: insar_conv1x1_out_fwd / _bwd / _wgrad / _wgrad_y), one launch at a time, against
tests/tail_ref.py. The operands are small integers (x in [-8, 8], w, bias, dlogits in [-4, 4]), so every logit, every dx element
and every folded partial sum is an integer that fp32 — and bf16 where it is stored — holds exactly under any summation order
(tests/test_tail_ref_host.py checks that for every case): the assertion is torch.equal. Outputs are prefilled with NaN: every
element that should be written is, the halo of dx and the channels outside a slice are not. One float case per path and dtype
exercises the rounding of the bf16 pack.

The narrow backward kernel's LDS passes 64 KB at bf16, C = 512, K = 7 or 8; the launchers raise the kernel's limit
(hipFuncAttributeMaxDynamicSharedMemorySize) and the shape runs: it is among the exact cases of _bwd and _wgrad. (The
runtime of ROCm 7.2 accepts the launch without the attribute as well — DESIGN.md "Testing the tail of the step".)"""
import pytest
import torch

from tests import tail_ref as tr
from tests.helpers import max_rel

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
E_SHAPE = -1001
CASES = tr.head_case_list()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _padded(x_nchw, dtype, dev, ctot=None, c_off=0, fill=float("nan")):
    """A padded NHWC buffer [B][H+2][W+2][ctot] filled with `fill`, x in the interior of the channel slice; and its Act."""
    from insar_unet_ca_amd.engine import Act
    B, C, H, W = x_nchw.shape
    ctot = ctot or C
    buf = torch.full((B, H + 2, W + 2, ctot), fill, dtype=dtype)
    buf[:, 1:-1, 1:-1, c_off:c_off + C] = x_nchw.permute(0, 2, 3, 1).to(dtype)
    buf = buf.to(dev)
    return buf, Act(buf, B, H, W, ctot, c_off, C)


def _empty_act(B, C, H, W, dtype, dev, ctot=None, c_off=0):
    from insar_unet_ca_amd.engine import Act
    ctot = ctot or C
    buf = torch.full((B, H + 2, W + 2, ctot), float("nan"), dtype=dtype, device=dev)
    return buf, Act(buf, B, H, W, ctot, c_off, C)


def _guarded(shape, dev, guard=16):
    """A NaN-filled float32 tensor of `shape` with `guard` sentinel floats behind it: (view, whole buffer)."""
    n = 1
    for d in shape:
        n *= d
    whole = torch.full((n + guard,), float("nan"), device=dev)
    whole[n:] = 7.0
    return whole[:n].view(shape), whole


def _guard_intact(whole, guard=16):
    return bool((whole[-guard:] == 7.0).all())


def _untouched_outside(buf, c_off, C):
    """The halo and the channels outside [c_off, c_off + C) of a NaN-prefilled buffer are still NaN."""
    t = buf.float().clone()
    t[:, 1:-1, 1:-1, c_off:c_off + C] = float("nan")
    return bool(torch.isnan(t).all())


def _interior(buf, c_off, C):
    return buf[:, 1:-1, 1:-1, c_off:c_off + C].permute(0, 3, 1, 2).double().cpu()


def _run_case(dev, c, dtype, ctot=None, c_off=0, wgrad=True):
    """fwd, bwd and (narrow inputs) wgrad on the case's operands; asserts the exact results."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    s = _lib.stream_ptr()
    B, C, H, W, K = c.B, c.C, c.H, c.W, c.K
    xbuf, xa = _padded(c.x, dtype, dev, ctot, c_off)
    w_d = c.w.float().to(dev)
    b_d = None if c.bias is None else c.bias.float().to(dev)
    dl_d = c.dl.float().to(dev)
    logits, lwhole = _guarded((B, K, H, W), dev)
    call("insar_conv1x1_out_fwd", xa.ref, ptr(w_d), ptr(b_d), ptr(logits), K, s)
    assert torch.equal(logits.double().cpu(), c.logits) and _guard_intact(lwhole)
    dxbuf, dxa = _empty_act(B, C, H, W, dtype, dev, ctot, c_off)
    nb = call("insar_conv1x1_out_bwd_blocks", B, H)
    assert nb == min(B * H, 1024)
    part, pwhole = _guarded((nb, K * C + K), dev)
    call("insar_conv1x1_out_bwd", xa.ref, ptr(w_d), ptr(dl_d), K, dxa.ref, ptr(part), s)
    assert torch.equal(_interior(dxbuf, c_off, C), c.dx) and _untouched_outside(dxbuf, c_off, C)
    assert bool(torch.isfinite(part).all()) and _guard_intact(pwhole)
    fold = part.double().sum(0).cpu()                       # integers below 2^24 each, below 2^53 in sum: exact
    assert torch.equal(fold[:K * C].view(K, C), c.dW) and torch.equal(fold[K * C:], c.db)
    if wgrad:
        part2, p2whole = _guarded((nb, K * C + K), dev)
        call("insar_conv1x1_out_wgrad", xa.ref, ptr(w_d), ptr(dl_d), K, ptr(part2), s)
        assert bool(torch.isfinite(part2).all()) and _guard_intact(p2whole)
        assert torch.equal(part2.double().sum(0).cpu(), fold)
    # the operands were only read
    assert torch.equal(_interior(xbuf, c_off, C), c.x) and _untouched_outside(xbuf, c_off, C)


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_head_exact_on_integer_operands(dev, case):
    cid, dt, C, K, (B, H, W), bias = CASES[case]
    c = tr.head_case(case, B, C, H, W, K, bias)
    tr.assert_head_case_exact(c)
    _run_case(dev, c, DT[dt], wgrad=not tr.is_wide(dt, C))


@pytest.mark.parametrize("dt,C", [("f32", 64), ("bf16", 256), ("f32", 260), ("bf16", 1024)])
def test_head_exact_on_a_channel_slice(dev, dt, C):
    """x and dx are the slice [16, 16 + C) of a buffer of C + 40 channels: nothing outside the slice is written."""
    c = tr.head_case(1000 + C, 2, C, 3, 5, 3, True)
    tr.assert_head_case_exact(c)
    _run_case(dev, c, DT[dt], ctot=C + 40, c_off=16, wgrad=not tr.is_wide(dt, C))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("gate", [True, False])
def test_head_wgrad_from_y_exact(dev, dt, gate):
    """insar_conv1x1_out_wgrad_y recomputes the head's input z = round_T(relu(y*scale + shift) * gate[n]) from integer y and
    power-of-two scale / gate values: z and every partial sum are exact."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    dtype = DT[dt]
    c = tr.fromy_case(7, 2, 64, 3, 5, 3, gate, dtype)
    tr.assert_fromy_case_exact(c, dtype)
    _, ya = _padded(c.y, dtype, dev)
    sc, sh = c.scale.float().to(dev), c.shift.float().to(dev)
    g_d = c.gate.float().contiguous().to(dev) if gate else None
    w_d, dl_d = c.w.float().to(dev), c.dl.float().to(dev)
    nb = call("insar_conv1x1_out_bwd_blocks", c.B, c.H)
    part, whole = _guarded((nb, c.K * c.C + c.K), dev)
    call("insar_conv1x1_out_wgrad_y", ya.ref, ptr(sc), ptr(sh), ptr(g_d), ptr(w_d), ptr(dl_d), c.K, ptr(part), _lib.stream_ptr())
    assert bool(torch.isfinite(part).all()) and _guard_intact(whole)
    fold = part.double().sum(0).cpu()
    assert torch.equal(fold[:c.K * c.C].view(c.K, c.C), c.dW) and torch.equal(fold[c.K * c.C:], c.db)
    # and the plain wgrad on z itself gives the same partial sums
    _, za = _padded(c.z, dtype, dev)
    part2, _ = _guarded((nb, c.K * c.C + c.K), dev)
    call("insar_conv1x1_out_wgrad", za.ref, ptr(w_d), ptr(dl_d), c.K, ptr(part2), _lib.stream_ptr())
    assert torch.equal(part2.double().sum(0).cpu(), fold)


@pytest.mark.parametrize("dt,C", [("f32", 64), ("bf16", 512), ("f32", 512), ("bf16", 520)])
@pytest.mark.parametrize("K", [0, 9])
def test_head_refuses_bad_class_counts_and_writes_nothing(dev, dt, C, K):
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import ptr
    lib = _lib.load()
    s = _lib.stream_ptr()
    dtype = DT[dt]
    B, H, W = 2, 3, 5
    _, xa = _padded(torch.ones(B, C, H, W), dtype, dev)
    dxbuf, dxa = _empty_act(B, C, H, W, dtype, dev)
    w_d, b_d, dl_d = torch.ones(9 * C, device=dev), torch.ones(9, device=dev), torch.ones(B * 9 * H * W, device=dev)
    sc = torch.ones(C, device=dev)
    logits, _ = _guarded((B * 9 * H * W,), dev)
    part, _ = _guarded((B * H, 9 * C + 9), dev)
    launches = [
        ("insar_conv1x1_out_fwd", lambda: lib.insar_conv1x1_out_fwd(xa.ref, ptr(w_d), ptr(b_d), ptr(logits), K, s)),
        ("insar_conv1x1_out_bwd", lambda: lib.insar_conv1x1_out_bwd(xa.ref, ptr(w_d), ptr(dl_d), K, dxa.ref, ptr(part), s)),
    ]
    if not tr.is_wide(dt, C):
        launches += [
            ("insar_conv1x1_out_wgrad", lambda: lib.insar_conv1x1_out_wgrad(xa.ref, ptr(w_d), ptr(dl_d), K, ptr(part), s)),
            ("insar_conv1x1_out_wgrad_y", lambda: lib.insar_conv1x1_out_wgrad_y(xa.ref, ptr(sc), ptr(sc), None, ptr(w_d), ptr(dl_d), K,
                                                                               ptr(part), s)),
        ]
    for name, fn in launches:
        assert fn() == E_SHAPE, name
        msg = lib.insar_last_error().decode()
        assert name in msg and "num_classes" in msg, msg
    torch.cuda.synchronize()
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(part).all()) and bool(torch.isnan(dxbuf.float()).all())


@pytest.mark.parametrize("dt,C", [("f32", 64), ("bf16", 256), ("f32", 512), ("bf16", 1024)])
def test_head_float_operands_against_float64(dev, dt, C):
    """Non-integer operands (exactly representable in the compute type), one case per path and dtype: logits and folded
    partial sums within 2e-5 of float64, dx within 2e-5 (fp32) / 1e-2 (stored bf16) — the bounds of test_deeplab_kernels_gpu."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    s = _lib.stream_ptr()
    dtype = DT[dt]
    gen = torch.Generator().manual_seed(C)
    B, H, W, K = 2, 6, 5, 3
    x = torch.randn((B, C, H, W), generator=gen).to(dtype).double()
    w, b = (0.05 * torch.randn((K, C), generator=gen)).double(), torch.randn((K,), generator=gen).double()
    dl = torch.randn((B, K, H, W), generator=gen).double()
    _, xa = _padded(x, dtype, dev)
    w_d, b_d, dl_d = w.float().to(dev), b.float().to(dev), dl.float().to(dev)
    logits, _ = _guarded((B, K, H, W), dev)
    call("insar_conv1x1_out_fwd", xa.ref, ptr(w_d), ptr(b_d), ptr(logits), K, s)
    dxbuf, dxa = _empty_act(B, C, H, W, dtype, dev)
    nb = call("insar_conv1x1_out_bwd_blocks", B, H)
    part, _ = _guarded((nb, K * C + K), dev)
    call("insar_conv1x1_out_bwd", xa.ref, ptr(w_d), ptr(dl_d), K, dxa.ref, ptr(part), s)
    dx, dW, db = tr.head_backward(x, w, dl)
    fold = part.double().sum(0).cpu()
    figs = (max_rel(logits, tr.head_forward(x, w, b)), max_rel(_interior(dxbuf, 0, C), dx),
            max_rel(fold[:K * C].view(K, C), dW), max_rel(fold[K * C:], db))
    print("head float %s C=%d: logits %.2e dx %.2e dW %.2e db %.2e" % ((dt, C) + figs))
    assert figs[0] <= 2e-5 and figs[1] <= (2e-5 if dt == "f32" else 1e-2) and figs[2] <= 2e-5 and figs[3] <= 2e-5
    assert _untouched_outside(dxbuf, 0, C)
