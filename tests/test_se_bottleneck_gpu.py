"""GPU: the SE-gated bottleneck of FCN-SE (fcn.SEBottleneckPlan: conv3 + bn3 statistics, insar_se_squeeze / insar_se_excite in
their no-ReLU mode, the gated residual apply insar_se_res_apply; backward through insar_bnrelu_bwd_reduce, insar_bnse_bwd_coef
and insar_bnrelu_bwd_apply) against tests/golden/g12_se_bottleneck.npz, which the reference's own BottleneckWithSE /
SEBlock produced (tools/gen_golden_fcn.py) around four blocks of its FCN-SE: layer1.0 (64 -> 256, downsample), layer2.0
(stride 2), layer3.1 (dilation 2) and layer4.1 (C = 2048, dilation 4), train and eval mode, two steps (BatchNorm buffers
after each). Tolerances are multiples of torch's own float32-vs-float64 noise stored with every value. Also: the new entry
point against torch elementwise at every chunk geometry, bf16, bitwise repeatability, and the wide output-conv path."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import closed_form as cf

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_se_bottleneck.npz")
CASES = {"l1b0": ("layer1", 0), "l2b0": ("layer2", 0), "l3b1": ("layer3", 1), "l4b1": ("layer4", 1)}
BLOCK_SEED, BLOCK_X_SEED, BLOCK_G_SEED = 3, 21, 5          # as tools/gen_golden_fcn.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def fcn_se():
    import insar_unet_ca_amd as iu
    torch.manual_seed(0)
    return iu.FCN_SingleChannel_SE(2)


def _block(fcn_se, tag, dev):
    import copy
    layer, idx = CASES[tag]
    blk = copy.deepcopy(fcn_se.model.backbone[layer][idx])
    blk.load_state_dict(cf.fill_state_dict_random(blk.state_dict(), seed=BLOCK_SEED))
    return blk.to(dev)


def run_block(blk, shape, training, dtype, dev, steps=2):
    """Forward + backward of one SEBottleneckPlan, as FCNPlan launches it; per step: out, dx, gradients, buffers."""
    from insar_unet_ca_amd.engine import Act, Ctx, GradSink, WeightSet, pack_input, unpack_output
    from insar_unet_ca_amd.fcn import SEBottleneckPlan
    blk.train(training)
    B, Cin, H, W = shape
    ctx = Ctx(dev, dtype)
    x = Act.alloc(B, H, W, Cin, dtype, dev)
    pack_input(cf.make_input_random(shape, seed=BLOCK_X_SEED).to(dev), x)
    plan = SEBottleneckPlan(ctx, blk, x, "blk")
    ws = WeightSet(ctx, [u.w for u in plan.units()])
    sink = GradSink(ctx, None, [plan.params()])
    dx = Act.alloc(B, H, W, Cin, dtype, dev)
    o = plan.out
    g = cf.make_input_random((B, o.c_len, o.H, o.W), seed=BLOCK_G_SEED).to(dev)
    names = {id(p): k for k, p in blk.named_parameters()}
    res = []
    for _ in range(steps):
        with ctx.side_stream():
            ws.refresh()
        ctx.join_side()
        plan.forward(training)
        out = unpack_output(plan.out)
        pack_input(g, plan.grad_out())
        dx.buf.zero_()
        plan.backward(sink, training, dx, None)
        ctx.join_side()
        torch.cuda.synchronize()
        r = {"out": out.cpu(), "dx": unpack_output(dx).cpu()}
        r.update({f"grad/{names[id(p)]}": sink.view(p).detach().cpu().clone() for p in plan.params()})
        r.update({f"buf/{k}": b.detach().cpu().clone() for k, b in blk.named_buffers() if not k.endswith("num_batches_tracked")})
        res.append(r)
    return res


def _check(gold, prefix, got, k, floor):
    """norm and 64 fixed samples of `got` against the stored float64 values: within k x torch's fp32 noise (+ floor) of
    the tensor's largest magnitude."""
    a = got.double().reshape(-1).numpy()
    absmax = float(gold[f"{prefix}/absmax"])
    tol = k * float(gold[f"{prefix}/noise"]) + floor
    ref_s = gold[f"{prefix}/samples"]
    err_s = float(np.abs(a[cf.sample_indices(a.size, 64)] - ref_s).max()) / max(absmax, 1e-30)
    norm = float(gold[f"{prefix}/norm"])
    err_n = abs(float(np.linalg.norm(a)) - norm) / max(norm, 1e-30)
    return max(err_s, err_n), tol


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("tag", list(CASES))
def test_se_bottleneck_fp32_against_the_reference(dev, gold, fcn_se, tag, training):
    """fp32: output, input gradient, every parameter gradient (conv / BatchNorm / the SE MLP's W1, W2) and the BatchNorm
    running statistics after each of two steps, against the reference's BottleneckWithSE."""
    shape = tuple(int(v) for v in gold[f"{tag}/shape"])
    mode = "train" if training else "eval"
    res = run_block(_block(fcn_se, tag, dev), shape, training, torch.float32, dev)
    bad, worst = {}, (0.0, None)
    for s, r in enumerate(res):
        for k, v in r.items():
            prefix = f"{tag}/{mode}/step{s}/{k}"
            if f"{prefix}/norm" not in gold:
                continue
            err, tol = _check(gold, prefix, v, 100, 2e-5)
            worst = max(worst, (err, prefix))
            if err > tol:
                bad[prefix] = (err, tol)
    print(f"{tag} {mode}: worst {worst[0]:.2e} at {worst[1]}")
    assert not bad, bad
    for k in ("grad/se_block.fc.0.weight", "grad/se_block.fc.2.weight", "grad/bn3.weight", "grad/bn3.bias", "out", "dx"):
        assert f"{tag}/{mode}/step0/{k}/norm" in gold, k


@pytest.mark.parametrize("tag", ["l1b0", "l2b0", "l4b1"])
def test_se_bottleneck_bf16(dev, gold, fcn_se, tag):
    """bf16 activations (fp32 gate, statistics and SE arithmetic) against the reference's float64 values. bf16 storage of y,
    the activations and the gradients is amplified by the BatchNorm backward (measured: output 2.5e-3, input gradient
    2-7e-2, SE weight gradients 0.6-6e-2, bn3 gradients 4-9e-2 of the largest magnitude); the gates sit at about twice
    that, far below the O(1) error of a misplaced chunk. C = 256 / 512 / 2048 bf16 run the gated apply with 8 / 4 / 1
    pixel lanes per work-group (test_se_res_apply_against_torch checks that kernel element by element)."""
    shape = tuple(int(v) for v in gold[f"{tag}/shape"])
    r = run_block(_block(fcn_se, tag, dev), shape, True, torch.bfloat16, dev, steps=1)[0]
    for k, tol in (("out", 1e-2), ("dx", 0.15), ("grad/se_block.fc.0.weight", 0.12), ("grad/se_block.fc.2.weight", 0.12),
                   ("grad/bn3.weight", 0.2), ("grad/bn3.bias", 0.2)):
        err, _ = _check(gold, f"{tag}/train/step0/{k}", r[k], 0, 0)
        print(f"{tag} bf16 {k}: {err:.2e}")
        assert err <= tol, (k, err)


def test_se_bottleneck_two_runs_bitwise(dev, fcn_se, gold):
    shape = tuple(int(v) for v in gold["l4b1/shape"])
    a = run_block(_block(fcn_se, "l4b1", dev), shape, True, torch.float32, dev, steps=1)[0]
    b = run_block(_block(fcn_se, "l4b1", dev), shape, True, torch.float32, dev, steps=1)[0]
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _act(t_nhwc_padded, B, H, W, C, code):
    from insar_unet_ca_amd import _lib
    return _lib.InsarAct(t_nhwc_padded.data_ptr(), B, H, W, C, 0, C, code, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [64, 256, 512, 1024, 2048])
def test_se_res_apply_against_torch(dev, C, dtype):
    """insar_se_res_apply = relu(gate[n][c] * (y * scale + shift) + res) at every chunk geometry (the block's pixel lanes
    from 8 down to 1, and several chunks per thread), halo left untouched."""
    from insar_unet_ca_amd import _lib
    g = torch.Generator().manual_seed(C)
    B, H, W = 2, 5, 7
    code = _lib.dtype_code(dtype)
    y = torch.randn(B, H + 2, W + 2, C, generator=g).to(dtype).to(dev)
    res = torch.randn(B, H + 2, W + 2, C, generator=g).to(dtype).to(dev)
    dst = torch.full((B, H + 2, W + 2, C), 7.0, dtype=dtype, device=dev)
    scale, shift = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    gate = torch.rand(B, C, generator=g).to(dev)
    ay, ar, ad = (_act(t, B, H, W, C, code) for t in (y, res, dst))
    _lib.call("insar_se_res_apply", ctypes.byref(ay), scale.data_ptr(), shift.data_ptr(), gate.data_ptr(), ctypes.byref(ar),
              ctypes.byref(ad), _lib.stream_ptr())
    torch.cuda.synchronize()
    s = gate[:, None, None, :]
    ref = torch.relu(s * (y.float() * scale + shift) + res.float())
    inner = (slice(None), slice(1, -1), slice(1, -1))
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    err = float(((dst[inner].float() - ref[inner]).abs() / (1.0 + ref[inner].abs())).max())
    assert err <= tol, err
    halo = dst.clone()
    halo[inner] = 7.0
    assert bool((halo.float() == 7.0).all())


@pytest.mark.parametrize("dtype,C", [(torch.float32, 512), (torch.bfloat16, 1024), (torch.float32, 256)])
def test_output_conv_wide_inputs_against_torch(dev, dtype, C):
    """insar_conv1x1_out_fwd / _bwd at inputs wider than one wave of chunks (the FCN head's 512 fp32 channels), against
    torch's 1x1 convolution: logits, input gradient and the per-block weight / bias partial sums."""
    from insar_unet_ca_amd import _lib
    g = torch.Generator().manual_seed(3)
    B, H, W, K = 2, 6, 5, 2
    code = _lib.dtype_code(dtype)
    x = torch.zeros(B, H + 2, W + 2, C, dtype=dtype)
    x[:, 1:-1, 1:-1] = torch.randn(B, H, W, C, generator=g).to(dtype)
    x = x.to(dev)
    w = (0.05 * torch.randn(K, C, generator=g)).to(dev)
    b = torch.randn(K, generator=g).to(dev)
    logits = torch.empty(B, K, H, W, device=dev)
    ax = _act(x, B, H, W, C, code)
    s = _lib.stream_ptr()
    _lib.call("insar_conv1x1_out_fwd", ctypes.byref(ax), w.data_ptr(), b.data_ptr(), logits.data_ptr(), K, s)
    xin = x[:, 1:-1, 1:-1].float().permute(0, 3, 1, 2)
    ref = F.conv2d(xin, w[:, :, None, None], b)
    torch.cuda.synchronize()
    assert float((logits - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    dl = torch.randn(B, K, H, W, generator=g).to(dev)
    dx = torch.zeros_like(x)
    adx = _act(dx, B, H, W, C, code)
    nb = _lib.call("insar_conv1x1_out_bwd_blocks", B, H)
    part = torch.zeros(nb, K * C + K, device=dev)
    _lib.call("insar_conv1x1_out_bwd", ctypes.byref(ax), w.data_ptr(), dl.data_ptr(), K, ctypes.byref(adx), part.data_ptr(), s)
    torch.cuda.synchronize()
    ref_dx = torch.einsum("bkhw,kc->bhwc", dl, w)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert float((dx[:, 1:-1, 1:-1].float() - ref_dx).abs().max()) <= tol * float(ref_dx.abs().max())
    ref_dw = torch.einsum("bkhw,bchw->kc", dl, xin)
    tot = part.sum(0)
    assert float((tot[:K * C].view(K, C) - ref_dw).abs().max()) <= 1e-4 * float(ref_dw.abs().max())
    assert float((tot[K * C:] - dl.sum((0, 2, 3))).abs().max()) <= 1e-4 * float(dl.abs().sum())
