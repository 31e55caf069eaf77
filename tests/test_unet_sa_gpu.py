"""GPU: the SA U-Net (`insar_unet_ca_amd.spatial.UNet`, Unet-SpatialAttention.py) end to end on the HIP path.

Tolerances
  fp32 logits     : <= 1e-3 max-rel against the float64 reference (north_star), train and eval.
  gradient norms  : |norm - ref| <= max(GRAD_K x torch's own fp32-vs-fp64 deviation of that norm, GRAD_FLOOR) x ref.
                    Two fp32 implementations disagree on the ReLU mask of pre-activations within rounding of 0 (see
                    tests/test_parity_gpu.py); the floor is the one the U-Net-CA gradient norms are held to there (5e-2).
  Adam trajectory : the 5 losses within ADAM_K x torch's own fp32-vs-fp64 deviation of the same trajectory.
  config 2 bf16   : against the fp32 HIP step, the gates tests/test_configs_gpu.py holds U-Net-CA to (5e-2, 98.5 %).
"""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import closed_form as cf
from tests.helpers import max_rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FWD_TOL = 1e-3
GRAD_K, GRAD_FLOOR = 50.0, 5e-2
ADAM_K = 2.0
BF16_TOL, BF16_ARGMAX = 5e-2, 0.985


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _net(dev, dtype=None, seed=7):
    import insar_unet_ca_amd as iu
    net = iu.UNetSpatialAttention(2, 2, compute_dtype=dtype)
    net.load_state_dict(cf.fill_state_dict_random(net.state_dict(), seed=seed))
    return net.to(dev)


def _inputs(dev):
    x = cf.make_input_random((2, 2, 64, 64), seed=11).to(dev)
    t = cf.make_target_random((2, 64, 64), seed=13, ignore_frac=0.05).to(dev)
    return x, t


def test_fp32_logits_gradients_and_adam_against_reference(dev, golden):
    import insar_unet_ca_amd as iu
    g = golden("g11_unet_sa")
    x, t = _inputs(dev)
    crit = iu.CrossEntropyLoss(ignore_index=255)
    net = _net(dev).train()
    logits = net(x)
    loss = crit(logits, t)
    loss.backward()
    ref = torch.from_numpy(g["train/logits/full"])
    err = max_rel(logits, ref)
    assert err <= FWD_TOL, err
    assert abs(float(loss) - float(g["train/loss/full"][0])) <= 1e-4 * abs(float(g["train/loss/full"][0]))
    worst = []
    for k, p in net.named_parameters():
        key = f"train/gradnorm/{k}"
        nrm, noise = float(g[f"{key}/full"][0]), float(g[f"{key}/noise"])
        got = float(p.grad.double().norm())
        if k.endswith(("double_conv.0.bias", "double_conv.3.bias")):
            continue                                     # pre-BatchNorm conv biases: zero gradient up to rounding
        tol = max(GRAD_K * noise, GRAD_FLOOR)
        assert abs(got - nrm) <= tol * nrm, f"{k}: {got} vs {nrm} (tol {tol:.2e})"
        worst.append((abs(got - nrm) / nrm, k))
    print("largest gradient-norm deviations:", sorted(worst)[-3:])
    # eval mode (running statistics)
    net_e = _net(dev).eval()
    with torch.no_grad():
        le = net_e(x)
    assert max_rel(le, torch.from_numpy(g["eval/logits/full"])) <= FWD_TOL
    # 5 Adam steps
    net_a = _net(dev).train()
    opt = iu.Adam(net_a.parameters(), lr=1e-4)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        l = crit(net_a(x), t)
        l.backward()
        opt.step()
        losses.append(float(l))
    exp = g["adam/loss/full"].astype(np.float64)
    # torch's own fp32 trajectory leaves the fp64 one by 1.5e-3 relative within these 5 steps (Adam amplifies the sign of
    # near-zero gradient elements): the gate is ADAM_K x that deviation
    tol = max(ADAM_K * float(g["adam/loss/noise"]), 1e-4)
    dev_rel = np.abs(np.array(losses) - exp).max() / np.abs(exp).max()
    print(f"Adam trajectory: max-rel {dev_rel:.2e} (torch fp32: {float(g['adam/loss/noise']):.2e})")
    assert dev_rel <= tol, (losses, exp)


def test_config2_bf16_step_tracks_fp32(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.data import make_batch
    x, y = (v.to(dev) for v in make_batch(0, 16, 256))
    crit = iu.CrossEntropyLoss(ignore_index=255)
    out = {}
    for dt in (torch.float32, torch.bfloat16):
        torch.manual_seed(3)
        net = iu.UNetSpatialAttention(2, 2, compute_dtype=dt).to(dev).train()
        opt = iu.Adam(net.parameters(), lr=1e-4)
        opt.zero_grad()
        logits = net(x)
        loss = crit(logits, y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        assert all(torch.isfinite(p.grad).all() for p in net.parameters())
        out[dt] = (logits.detach().clone(), float(loss))
        del net, opt, logits, loss
        torch.cuda.empty_cache()
    l32, l16 = out[torch.float32][0], out[torch.bfloat16][0]
    err = max_rel(l16, l32)
    agree = (l16.argmax(1) == l32.argmax(1)).float().mean().item()
    print(f"config 2 SA bf16 vs fp32: logits max-rel {err:.3e}, arg-max agreement {agree:.4f}")
    assert err <= BF16_TOL and agree >= BF16_ARGMAX


def _train(dev, steps, dtype=torch.bfloat16, tape_mode=None, monkeypatch=None, eval_at=(), reassign_at=None):
    """`steps` training steps; a no-grad eval forward after each step in `eval_at` (the plan's eager path, between tape
    replays); new storage under every parameter and BatchNorm buffer before step `reassign_at`."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import tape
    from insar_unet_ca_amd.data import make_batch
    if tape_mode is not None:
        monkeypatch.setattr(tape, "MODE", tape_mode)
    torch.manual_seed(4)
    net = iu.UNetSpatialAttention(2, 2, compute_dtype=dtype).to(dev).train()
    crit = iu.DiceCELoss(ignore_index=255)
    opt = iu.Adam(net.parameters(), lr=1e-3)
    batches = [tuple(v.to(dev) for v in make_batch(4 * i, 4, 64)) for i in range(3)]
    losses, evals = [], []
    for i in range(steps):
        if reassign_at is not None and i == reassign_at:
            for prm in net.parameters():
                prm.data = prm.data.clone()
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean = m.running_mean.clone()
                    m.running_var = m.running_var.clone()
        x, y = batches[i % 3]
        opt.zero_grad(set_to_none=True)
        loss = crit(net(x), y)
        loss.backward()
        opt.step()
        losses.append(float(loss))
        if i in eval_at:
            net.eval()
            with torch.no_grad():
                evals.append(net(batches[0][0]).clone())
            net.train()
    torch.cuda.synchronize()
    plans = [pl for lst in net._plans.plans.values() for pl in lst]
    reports = [pl.tape_report() for pl in plans if hasattr(pl, "tape_report")]
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    state.update({f"eval{j}": e for j, e in enumerate(evals)})
    return losses, state, reports


def _same(a, b):
    assert a[0] == b[0]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_two_fresh_runs_are_bitwise_equal(dev):
    _same(_train(dev, 6), _train(dev, 6))


def test_launch_tape_replay_matches_eager(dev, monkeypatch):
    taped = _train(dev, 6, tape_mode="1", monkeypatch=monkeypatch)
    eager = _train(dev, 6, tape_mode="0", monkeypatch=monkeypatch)
    print("tape reports:", taped[2])
    _same(taped, eager)
    assert any(v.startswith("replaying") for r in taped[2] for v in r.values()), taped[2]


def test_launch_tape_with_eval_passes_and_reassigned_storage_matches_eager(dev, monkeypatch):
    """Training until the tape replays, an eval forward (eager, BatchNorm on running statistics) between replays, more
    training, new parameter / buffer storage, more training: bit for bit the run without tapes. The SA units' launch
    descriptors must not carry the eval pass's mode or a stale parameter pointer into the replayed training steps."""
    kw = dict(eval_at=(5, 7, 11), reassign_at=9)
    taped = _train(dev, 13, tape_mode="1", monkeypatch=monkeypatch, **kw)
    eager = _train(dev, 13, tape_mode="0", monkeypatch=monkeypatch, **kw)
    print("tape reports:", taped[2])
    _same(taped, eager)
    assert any(v.startswith("replaying") for r in taped[2] for v in r.values()), taped[2]


def test_graphed_train_step_matches_eager(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.data import make_batch
    batches = [tuple(v.to(dev) for v in make_batch(4 * i, 4, 64)) for i in range(2)]

    def fresh():
        torch.manual_seed(6)
        net = iu.UNetSpatialAttention(2, 2, compute_dtype=torch.bfloat16).to(dev).train()
        return net, iu.CrossEntropyLoss(ignore_index=255), iu.Adam(net.parameters(), lr=1e-3)

    net, crit, opt = fresh()
    step = iu.GraphedTrainStep(net, crit, opt, batches[0][0], batches[0][1], warmup=2)
    lg = float(step(*batches[1]))
    sd_g = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net, crit, opt = fresh()
    for i in range(3):
        x, y = batches[0] if i < 2 else batches[1]
        opt.zero_grad(set_to_none=True)
        l = crit(net(x), y)
        l.backward()
        opt.step()
    torch.cuda.synchronize()
    assert float(l) == lg
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd_g[k]), k


def _names(net, x, y, crit):
    from insar_unet_ca_amd import _lib, tape
    old_mode = tape.MODE
    tape.MODE = "0"
    _lib._TAPE = []
    try:
        crit(net(x), y).backward()
        torch.cuda.synchronize()
        return [e[2] for e in _lib._TAPE]
    finally:
        _lib._TAPE = None
        tape.MODE = old_mode


def test_launch_sequence_is_the_plain_unet_plus_the_sa_units(dev):
    """The SA net launches exactly what UNet(use_se=False) launches, with the SA units' passes inserted; the U-Net
    launches none of them."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.data import make_batch
    x, y = (v.to(dev) for v in make_batch(0, 2, 64))
    crit = iu.CrossEntropyLoss(ignore_index=255)
    plain = _names(iu.UNet(2, 2, False).to(dev).train(), x, y, crit)
    ca = _names(iu.UNet(2, 2, True).to(dev).train(), x, y, crit)
    sa = _names(iu.UNetSpatialAttention(2, 2).to(dev).train(), x, y, crit)
    assert not any(n.startswith("insar_sa_") for n in plain + ca)
    stripped, prev = [], None
    for n in sa:
        if not (n.startswith("insar_sa_") or (n == "insar_bn_finalize" and prev == "insar_sa_conv")):
            stripped.append(n)
        prev = n
    assert stripped == plain
    assert sum(n.startswith("insar_sa_") for n in sa) == 4 * (4 + 7)


def test_checkpoint_interchange_with_the_contract(dev, golden):
    import insar_unet_ca_amd as iu
    with open(os.path.join(ROOT, "tests", "golden", "g11_unet_sa_contract.json")) as f:
        contract = json.load(f)
    sd = OrderedDict((k, torch.zeros(s, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32))
                     for k, s in zip(contract["keys"], contract["shapes"]))
    sd = cf.fill_state_dict_random(sd, seed=9)
    net = iu.UNetSpatialAttention(2, 2).to(dev)
    net.load_state_dict(sd, strict=True)
    back = net.state_dict()
    assert list(back.keys()) == contract["keys"]
    for k in sd:
        assert torch.equal(back[k].cpu(), sd[k]), k
    x, _ = _inputs(dev)
    with torch.no_grad():
        assert torch.isfinite(net.eval()(x)).all()
    other = iu.UNetSpatialAttention(2, 2)
    other.load_state_dict({k: v.cpu() for k, v in back.items()}, strict=True)


# ---- DataParallel: 2 ranks over gloo on one GPU ---------------------------------------------------------------------
def _dp_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.data import make_batch
    from insar_unet_ca_amd.parallel import DataParallel, ShardedAdam

    dev = torch.device("cuda:0")
    crit = iu.CrossEntropyLoss(ignore_index=255)
    x, y = (v.to(dev) for v in make_batch(rank * 2, 2, 64))
    res = {}
    # all-reduce path: gradients = mean of the ranks' local gradients
    torch.manual_seed(100 + rank)
    net = iu.UNetSpatialAttention(2, 2).to(dev).train()
    model = DataParallel(net, bucket_mb=4.0)
    hooks = dict(net._hooks)
    net._hooks.clear()
    crit(net(x), y).backward()
    res["local"] = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
    net._hooks.update(hooks)
    opt = iu.Adam(net.parameters(), lr=1e-3)
    trail = []
    for step in range(2):
        opt.zero_grad()
        loss = crit(model(x), y)
        loss.backward()
        if step == 0:
            res["reduced"] = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
        opt.step()
        trail.append(float(loss))
    torch.cuda.synchronize()
    res["allreduce"] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    res["allreduce_loss"] = trail
    # sharded path (reduce-scatter, sharded Adam, parameter all-gather) from the same start
    torch.manual_seed(100 + rank)
    net = iu.UNetSpatialAttention(2, 2).to(dev).train()
    dp = DataParallel(net, bucket_mb=4.0, shard_optimizer=True)
    hooks = dict(net._hooks)
    net._hooks.clear()
    crit(net(x), y).backward()                         # the same dry pass: BatchNorm buffers advance identically
    net.zero_grad(set_to_none=True)
    net._hooks.update(hooks)
    opt = ShardedAdam(dp, lr=1e-3)
    trail = []
    for step in range(2):
        opt.zero_grad()
        loss = crit(dp(x), y)
        loss.backward()
        opt.step()
        trail.append(float(loss))
    dp.params_ready()
    torch.cuda.synchronize()
    res["sharded"] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    res["sharded_loss"] = trail
    # SyncBN is refused for this net
    try:
        DataParallel(iu.UNetSpatialAttention(2, 2).to(dev), sync_bn=True)
        res["sync_bn"] = "accepted"
    except iu.InsarError as e:
        res["sync_bn"] = str(e)
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_two_ranks(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    import torch.multiprocessing as mp
    port = 29700 + (os.getpid() % 1000)
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    for k in r0["local"]:
        mean = 0.5 * (r0["local"][k] + r1["local"][k])
        scale = float(mean.abs().max()) + 1e-12
        assert float((r0["reduced"][k] - mean).abs().max()) <= 1e-5 * scale + 1e-9, k
        assert torch.equal(r0["reduced"][k], r1["reduced"][k]), k
    # the sharded path computes what the all-reduce path computes: losses and BatchNorm buffers bit for bit, parameters bit
    # for bit where the two optimizers run the same code. Adam's kernel (loss_optim.hip) updates a tensor's last numel % 4
    # elements in a scalar tail and the rest as float4; iu.Adam walks each parameter on its own, ShardedAdam the flat shard,
    # so a parameter whose size is not a multiple of 4 (the SA units' 1- and 9-element tensors, outc.bias) takes the tail in
    # one optimizer and the float4 body in the other. The two do not round alike: tools/adam_tail_paths.py runs the same
    # 4096 elements through both, and v ends up 1 ulp apart for 83 of them, p for 1 (profiles/r05_adam_tail_paths.txt).
    # Those parameters agree to an ulp-level tolerance; every other tensor bit for bit.
    for r in (r0, r1):
        assert r["allreduce_loss"] == r["sharded_loss"]
        for k in r["allreduce"]:
            a, b = r["allreduce"][k], r["sharded"][k]
            if k in r["local"] and a.numel() % 4:
                assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max()) + 1e-12, k
            else:
                assert torch.equal(a, b), k
    # the replicas' parameters stay identical (BatchNorm statistics are per replica without sync_bn)
    for k in r0["local"]:
        assert torch.equal(r0["allreduce"][k], r1["allreduce"][k]), k
    assert "sync_bn" in r0["sync_bn"] and "SA U-Net" in r0["sync_bn"]
