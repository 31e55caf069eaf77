"""GPU: results do not depend on which queue a launch sits on, and not on the optimizer's chunk size — bit for bit.

One training step of iu.UNet(2, 2, True) (forward, DiceCELoss, backward, Adam step; 3 x 48 x 48, fp32 and bf16) under
INSAR_SIDE_STREAM=0, PREP_SIDE=False and SMALL_WGRAD_MAIN=False against the default placement. The placement changes the
fill a weight gradient aims at and through it nsplit, so all five fill constants are pinned to one value in both runs;
SMALL_WGRAD_MAIN=False also leaves the first layer's fused apply + weight-gradient kernel, so SMALL_WGRAD_FUSE is off in
both runs of that case. Each case first shows from the launch record (tests/helpers.record_calls) that the two runs issue
the same entry points with the same integer arguments in the same order and that the variant really moved launches to
another stream; then every parameter gradient and every updated parameter is compared bitwise. One run per variant: a
missing event edge shows as a difference or not at all, nothing is repeated.

optim.CHUNK at 1024 and at 1000 (no divisor of the largest parameter): updated parameters and both moments bitwise equal
to the default chunk's.

The DeepLabV3-CA net (2 x 1 x 64 x 64, dropout off: the plan draws its own mask) takes the same step under
INSAR_SIDE_STREAM=0. Its plan reads neither PREP_SIDE (the weight re-layout always sits on the side stream there) nor
SMALL_WGRAD_MAIN (its stem is not the U-Net's direct first layer): those two would change nothing in it, so they have no
DeepLab case."""
import pytest
import torch

from tests.helpers import record_calls, small_ints

pytestmark = pytest.mark.gpu

_FILLS = ("WGRAD_FILL", "WGRAD_FILL_SMALL", "WGRAD_FILL_T", "WGRAD_FILL_DL", "WGRAD_FILL_ALONE")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()                      # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _step(dev, monkeypatch, dtype, deeplab=False):
    """One training step under the switches as they stand: (launch record, main stream, gradients, parameters, moments)."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd.data import make_batch
    x, y = make_batch(7, 2, 64, channels=1) if deeplab else make_batch(7, 3, 48)
    x, y = x.to(dev), y.to(dev)
    torch.manual_seed(11)
    if deeplab:
        net = iu.DeepLabV3_SingleChannel_Attn(num_classes=2, backbone="resnet50", pretrained=False, compute_dtype=dtype)
        net.aspp.project[3].p = 0.0
        net = net.to(dev).train()
    else:
        net = iu.UNet(2, 2, True, compute_dtype=dtype).to(dev).train()
    opt = iu.Adam(net.parameters(), lr=1e-3)
    log = record_calls(monkeypatch)
    main = _lib.stream_ptr()
    loss = iu.DiceCELoss(ignore_index=255)(net(x), y)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in net.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    frozen = list(log)
    params = {n: p.detach().clone() for n, p in net.named_parameters()}
    moments = {n: (opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for n, p in net.named_parameters()}
    # (a conv bias in front of a BatchNorm has a gradient of exactly zero: only the weights are asked to be non-zero)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert all(float(g.abs().max()) > 0 for n, g in grads.items() if n.endswith("weight"))
    return frozen, main, grads, params, moments


def _bitwise(a, b, what):
    bad = [n for n in a if not torch.equal(a[n].view(torch.int32), b[n].view(torch.int32))]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, first {bad[:6]}"


def _same_launches(base, var, what):
    def ints(args, stream):
        # the trailing stream handle is where the runs are meant to differ; the default stream's is 0, so a trailing 0 goes
        # too (a query's last argument that is 0 in one run and not in the other still shows: the tuples differ in length)
        return small_ints(args[:-1] if args and isinstance(args[-1], int) and args[-1] in (stream, 0) else args)
    a = [(n, ints(args, s)) for n, args, s in base]
    b = [(n, ints(args, s)) for n, args, s in var]
    first = next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), None)
    assert first is None and len(a) == len(b), \
        f"{what}: launch records differ at call {first}: {a[first] if first is not None else len(a)} vs {b[first] if first is not None else len(b)}"


def _off_main(log, main):
    return [n for n, _, s in log if s != main]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["INSAR_SIDE_STREAM=0", "PREP_SIDE=0", "SMALL_WGRAD_MAIN=0"])
def test_stream_placement_is_bitwise_neutral(dev, monkeypatch, variant, dtype):
    from insar_unet_ca_amd import engine
    monkeypatch.delenv("INSAR_SIDE_STREAM", raising=False)
    for k in _FILLS:
        monkeypatch.setattr(engine, k, 0.5)
    if variant == "SMALL_WGRAD_MAIN=0":
        monkeypatch.setattr(engine, "SMALL_WGRAD_FUSE", False)
    base_log, base_main, g0, p0, _ = _step(dev, monkeypatch, dtype)
    assert "insar_wgrad_reduce" in _off_main(base_log, base_main), "the default step runs its weight gradients on the side stream"
    if variant == "INSAR_SIDE_STREAM=0":
        monkeypatch.setenv("INSAR_SIDE_STREAM", "0")
    elif variant == "PREP_SIDE=0":
        monkeypatch.setattr(engine, "PREP_SIDE", False)
    else:
        monkeypatch.setattr(engine, "SMALL_WGRAD_MAIN", False)
    var_log, var_main, g1, p1, _ = _step(dev, monkeypatch, dtype)
    _same_launches(base_log, var_log, variant)
    # the variant really moved launches
    if variant == "INSAR_SIDE_STREAM=0":
        assert not _off_main(var_log, var_main)
    elif variant == "PREP_SIDE=0":
        assert "insar_weight_prep_pair_batch" in _off_main(base_log, base_main)
        assert "insar_weight_prep_pair_batch" not in _off_main(var_log, var_main)
    else:
        assert "insar_conv3x3_small_wgrad" not in _off_main(base_log, base_main)
        assert "insar_conv3x3_small_wgrad" in _off_main(var_log, var_main)
    _bitwise(g0, g1, variant + " gradients")
    _bitwise(p0, p1, variant + " updated parameters")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_deeplab_step_without_a_side_stream_is_bitwise(dev, monkeypatch, dtype):
    from insar_unet_ca_amd import engine
    monkeypatch.delenv("INSAR_SIDE_STREAM", raising=False)
    for k in _FILLS:
        monkeypatch.setattr(engine, k, 0.5)
    base_log, base_main, g0, p0, _ = _step(dev, monkeypatch, dtype, deeplab=True)
    moved = set(_off_main(base_log, base_main))
    assert {"insar_wgrad", "insar_wgrad_reduce", "insar_weight_prep_pair_batch"} <= moved, sorted(moved)
    monkeypatch.setenv("INSAR_SIDE_STREAM", "0")
    var_log, var_main, g1, p1, _ = _step(dev, monkeypatch, dtype, deeplab=True)
    _same_launches(base_log, var_log, "DeepLabV3-CA INSAR_SIDE_STREAM=0")
    assert not _off_main(var_log, var_main)
    _bitwise(g0, g1, "DeepLabV3-CA gradients")
    _bitwise(p0, p1, "DeepLabV3-CA updated parameters")


@pytest.mark.parametrize("chunk", [1024, 1000])
def test_adam_chunk_size_is_bitwise_neutral(dev, monkeypatch, chunk):
    from insar_unet_ca_amd import optim
    assert optim.CHUNK == 8192
    _, _, _, p0, m0 = _step(dev, monkeypatch, torch.float32)
    largest = max(v.numel() for v in p0.values())
    assert largest > 8192 and (chunk == 1024 or largest % chunk)
    monkeypatch.setattr(optim, "CHUNK", chunk)
    log, _, _, p1, m1 = _step(dev, monkeypatch, torch.float32)
    steps = [a for n, a, _ in log if n == "insar_adam_step"]
    assert steps and all(a[3] == chunk for a in steps), "the step was not launched with the chunk size under test"
    _bitwise(p0, p1, f"CHUNK={chunk} parameters")
    _bitwise({k: v[0] for k, v in m0.items()}, {k: v[0] for k, v in m1.items()}, f"CHUNK={chunk} exp_avg")
    _bitwise({k: v[1] for k, v in m0.items()}, {k: v[1] for k, v in m1.items()}, f"CHUNK={chunk} exp_avg_sq")
