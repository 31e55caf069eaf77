"""GPU: the SpatialAttention kernels (csrc/spatial_attn.hip) and the stand-alone `spatial.SpatialAttention` module.

Tolerances
  compress      : mean against float64 torch within fp32 summation noise (2e-6 of the channel values' scale); the maximum
                  and the first arg-max exactly.
  block, fp32   : against the float64 reference (tests/golden/g11_sa_block.npz, tools/gen_golden_sa.py), every tensor within
                  NOISE_K x torch's own fp32-vs-fp64 deviation on the same fixture (stored as `<key>/noise`), floor 1e-5.
  block, bf16   : operands rounded to bf16 at the module boundary (arithmetic in fp32): max-rel <= 3e-2 on the output;
                  rel-L2 <= 0.1 on the input gradient and <= 0.4 on the parameter gradients. A ReLU mask of the 1-channel
                  map that flips under bf16 rounding moves d_max of that pixel by O(1), so max-rel of dx is not a useful
                  figure: torch's own bf16 run of these fixtures has dx max-rel 0.17-0.28, rel-L2 0.04-0.07, and parameter
                  gradients rel-L2 up to 0.28 (BN2 bias) and 1.0 (BN1 weight) on c128, train; the HIP path measures <= 0.27.
                  Conv biases before a training-mode BatchNorm are skipped. Step 0 is compared element by element
                  everywhere (the C = 1024 output and input gradient from g11_sa_block_full).
"""

import numpy as np
import pytest
import torch

from oracle import closed_form as cf
from tests.helpers import to_np

pytestmark = pytest.mark.gpu

NOISE_K = 50.0
NOISE_FLOOR = 1e-5
BF16_OUT_TOL, BF16_DX_L2, BF16_GRAD_L2 = 3e-2, 0.1, 0.4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _gen():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_golden_sa.py")
    spec = importlib.util.spec_from_file_location("gen_golden_sa", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()


def _unit(dtype, dev, x: torch.Tensor):
    """An SAUnit on a fresh concat buffer holding x (NCHW); returns (unit, x Act)."""
    from insar_unet_ca_amd import spatial
    from insar_unet_ca_amd.engine import Act, Ctx, SAUnit, pack_input
    b, c, h, w = x.shape
    sa = spatial.SpatialAttention().to(dev)
    ctx = Ctx(dev, dtype)
    xa, ya = Act.alloc(b, h, w, c, dtype, dev), Act.alloc(b, h, w, c, dtype, dev)
    pack_input(x.to(dev), xa)
    return SAUnit(ctx, sa, xa, ya, "sa"), xa


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cn", [128, 256, 512, 1024])
def test_compress_against_float64(dev, dtype, cn):
    x = cf.make_input_random((2, cn, 12, 20), seed=cn)
    unit, xa = _unit(dtype, dev, x)
    unit.forward(True)
    torch.cuda.synchronize()
    xr = xa.nchw().double().cpu()                        # the operand as the kernel saw it (bf16-rounded in bf16)
    mean = xr.mean(1)
    mx, arg = xr.max(1)
    comp = unit.comp.cpu()
    assert (comp[:, 1:-1, 1:-1, 0].double() - mean).abs().max().item() <= 2e-6 * xr.abs().max().item()
    assert torch.equal(comp[:, 1:-1, 1:-1, 1].double(), mx)
    got_arg = (unit.arg.cpu().to(torch.int64) & 0xFFFF).view(2, 12, 20)
    assert torch.equal(got_arg, arg)
    # the halo stays zero (it pads the 3x3 stencils)
    halo = comp.clone()
    halo[:, 1:-1, 1:-1, :] = 0
    assert float(halo.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_compress_tie_picks_first_channel(dev, dtype):
    b, cn, h, w = 2, 64, 6, 10
    x = torch.round(cf.make_input((b, cn, h, w), 0.3) * 4.0) / 4.0
    # and a planted tie at known channels: every pixel's maximum 3.0 at channels 5, 17 and 40 (the first must win)
    x[:, [5, 17, 40]] = 3.0
    x[0, :, 0, 0] = 1.0                                   # all channels equal: channel 0
    unit, xa = _unit(dtype, dev, x)
    unit.forward(True)
    torch.cuda.synchronize()
    got = (unit.arg.cpu().to(torch.int64) & 0xFFFF).view(b, h, w)
    exp = torch.full((b, h, w), 5, dtype=torch.int64)
    exp[0, 0, 0] = 0
    assert torch.equal(got, exp)
    assert torch.equal(got, x.max(1).indices)             # torch's own rule on the same tensor


def test_channel_count_must_be_a_multiple_of_8(dev):
    import insar_unet_ca_amd as iu
    sa = iu.SpatialAttention().to(dev)
    with pytest.raises(iu.InsarError, match="multiple of 8"):
        sa(torch.zeros(1, 12, 8, 8, device=dev))


def _case(g, tag):
    shape = tuple(int(v) for v in g[f"{tag}/shape"])
    return shape, bool(int(g[f"{tag}/training"])), ("ties" if tag.startswith("ties") else "sep")


def _run_block(dev, dtype, shape, training, kind):
    import insar_unet_ca_amd as iu
    sa = iu.SpatialAttention()
    sa.load_state_dict(GEN.sa_state(sa))
    sa = sa.to(dev).train(training)
    sa.compute_dtype = dtype
    x0, g = GEN.block_input(shape, kind).to(dev), GEN.block_grad(shape).to(dev)
    steps = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        for p in sa.parameters():
            p.grad = None
        out = sa(x)
        out.backward(g)
        torch.cuda.synchronize()
        st = {"out": out.detach().cpu(), "dx": x.grad.cpu()}
        st.update({f"grad/{k}": p.grad.cpu().clone() for k, p in sa.named_parameters()})
        st.update({f"buf/{k}": b.cpu().clone() for k, b in sa.named_buffers() if not k.endswith("num_batches_tracked")})
        st["nbt"] = int(sa.compress_and_map.double_conv[1].num_batches_tracked)
        steps.append(st)
    return steps


def _ref(g, key, full=None):
    """The whole reference tensor: in g11_sa_block, or (step-0 output and input gradient of the C = 1024 cases) in
    g11_sa_block_full; None for the tensors stored as samples + norm only."""
    for store in (g, full):
        if store is not None and f"{key}/full" in store.files:
            return store[f"{key}/full"].astype(np.float64).reshape(-1)
    return None


def _check(g, key, got, tol, full=None):
    """max-rel against the whole reference tensor (or the 64 stored samples + the norm for the step-1 tensors of the
    C = 1024 cases, which repeat step 0's)."""
    a = to_np(got).astype(np.float64).reshape(-1)
    scale = max(float(g[f"{key}/absmax"]), 1e-30)
    ref = _ref(g, key, full)
    if ref is not None:
        err = float(np.abs(a - ref).max()) / scale
    else:
        idx = cf.sample_indices(a.size, 64)
        err = float(np.abs(a[idx] - g[f"{key}/samples"].astype(np.float64)).max()) / scale
        nrm = float(g[f"{key}/norm"])
        err = max(err, abs(float(np.sqrt((a * a).sum())) - nrm) / max(nrm, 1e-30))
    assert err <= tol, f"{key}: max-rel {err:.3e} > {tol:.3e}"
    return err


CASES = ["c128_train", "c128_eval", "c1024_train", "c1024_eval", "ties_train"]


@pytest.mark.parametrize("tag", CASES)
def test_block_fp32_against_reference(dev, golden, tag):
    g, full = golden("g11_sa_block"), golden("g11_sa_block_full")
    shape, training, kind = _case(g, tag)
    steps = _run_block(dev, torch.float32, shape, training, kind)
    worst = 0.0
    for s, st in enumerate(steps):
        for k, v in st.items():
            if k == "nbt":
                assert v == (s + 1 if training else 0)
                continue
            key = f"{tag}/step{s}/{k}"
            noise = float(g[f"{key}/noise"])
            if k.endswith(("0.bias", "3.bias")) and k.startswith("grad/") and training:
                # d(conv bias) before a training-mode BatchNorm is zero up to rounding: on the scale of its weight gradient
                wkey = key.replace(".bias", ".weight")
                tol = NOISE_K * 1e-6 * float(g[f"{wkey}/absmax"]) * shape[0] * shape[2] * shape[3]
                assert float(v.abs().max()) <= tol, f"{key}: {float(v.abs().max()):.3e} > {tol:.3e}"
                continue
            if s == 0 and k in ("out", "dx"):
                assert _ref(g, key, full) is not None, key          # every element of step 0 is checked
            err = _check(g, key, v, max(NOISE_K * noise, NOISE_FLOOR), full)
            worst = max(worst, err / max(noise, 1e-12))
    print(f"{tag}: worst error / torch's own fp32 noise = {worst:.1f}")


@pytest.mark.parametrize("tag", ["c128_train", "c1024_train", "c1024_eval"])
def test_block_bf16_against_reference(dev, golden, tag):
    g, full = golden("g11_sa_block"), golden("g11_sa_block_full")
    shape, training, kind = _case(g, tag)
    st = _run_block(dev, torch.bfloat16, shape, training, kind)[0]
    errs = {}
    for k, v in st.items():
        if k == "nbt" or k.startswith("buf/"):
            continue
        key = f"{tag}/step0/{k}"
        if k.endswith(("0.bias", "3.bias")) and k.startswith("grad/") and training:
            continue
        ref = _ref(g, key, full)
        assert ref is not None, key                      # step 0: every tensor is stored whole
        if k == "out":
            errs[k] = _check(g, key, v, BF16_OUT_TOL, full)
            continue
        a = v.double().reshape(-1).numpy()
        errs[k] = float(np.sqrt(((a - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum()))
        assert errs[k] <= (BF16_DX_L2 if k == "dx" else BF16_GRAD_L2), (k, errs[k])
    print(tag, {k: f"{e:.2e}" for k, e in errs.items()})


def test_block_rejects_cpu_tensors():
    import insar_unet_ca_amd as iu
    with pytest.raises(iu.InsarError, match="ROCm device"):
        iu.SpatialAttention()(torch.zeros(1, 8, 4, 4))


def test_block_is_bitwise_reproducible(dev):
    shape = (2, 256, 16, 16)
    a = _run_block(dev, torch.bfloat16, shape, True, "sep")
    b = _run_block(dev, torch.bfloat16, shape, True, "sep")
    for s in range(2):
        for k in a[s]:
            if k != "nbt":
                assert torch.equal(a[s][k], b[s][k]), k
