"""GPU: DataParallel over the FCN-SE plan (fcn.FCNPlan), two ranks over gloo on one GPU at the geometry of
tests/test_dp_gpu.py (2 tiles of 64 x 64 per rank): the bucketed all-reduce leaves the mean of the ranks' local gradients,
the sharded path (reduce-scatter, ShardedAdam, all-gather) computes what the all-reduce path computes, and sync_bn=True is
refused."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _make(iu, dev, rank):
    torch.manual_seed(100 + rank)                      # different init per rank: the broadcast must fix it
    net = iu.FCN_SingleChannel_SE(2).to(dev).train()
    net.model.classifier[3].p = 0.0                    # the dropout mask is per replica: compare without it
    return net


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
    x, y = make_batch(rank * 2, 2, 64, channels=1)
    x, y = x.to(dev), y.to(dev)
    res = {}
    net = _make(iu, dev, rank)
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
        trail.append(float(loss.detach()))
    torch.cuda.synchronize()
    res["allreduce"] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    res["allreduce_loss"] = trail
    net = _make(iu, dev, rank)
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
        trail.append(float(loss.detach()))
    dp.params_ready()
    torch.cuda.synchronize()
    res["sharded"] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    res["sharded_loss"] = trail
    try:
        DataParallel(iu.FCN_SingleChannel_SE(2).to(dev), sync_bn=True)
        res["sync_bn"] = "accepted"
    except iu.InsarError as e:
        res["sync_bn"] = str(e)
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_fcn_se_data_parallel_two_ranks(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    import torch.multiprocessing as mp
    port = 29800 + (os.getpid() % 1000)
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    for k in r0["local"]:
        mean = 0.5 * (r0["local"][k] + r1["local"][k])
        scale = float(mean.abs().max()) + 1e-12
        assert float((r0["reduced"][k] - mean).abs().max()) <= 1e-5 * scale + 1e-9, k
        assert torch.equal(r0["reduced"][k], r1["reduced"][k]), k
    # sharded == all-reduce: losses and BatchNorm buffers bit for bit; parameters bit for bit except where Adam's scalar
    # tail and float4 body round differently (parameters whose size is not a multiple of 4: see tests/test_unet_sa_gpu.py)
    for r in (r0, r1):
        assert r["allreduce_loss"] == r["sharded_loss"]
        for k in r["allreduce"]:
            a, b = r["allreduce"][k], r["sharded"][k]
            if k in r["local"] and a.numel() % 4:
                assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max()) + 1e-12, k
            else:
                assert torch.equal(a, b), k
        assert "sync_bn=True" in r["sync_bn"], r["sync_bn"]
    for k in r0["local"]:
        assert torch.equal(r0["allreduce"][k], r1["allreduce"][k]), k
