"""Augmentation and TTA on one GPU, in one process. Three sections, each interleaved round by round with what it is compared to:

(a) us per insar_aug_apply call on config 2's batch (16 x 2 x 256 x 256 float32 images + masks, int64 and uint8 source) for
    four tables (all-identity, flips only, full D4, full D4 with noise), the bytes each case moves and the achieved GB/s,
    next to the same transform written in torch ops;
(b) ms/step of a U-Net-CA bf16 training loop fed by DevicePrefetcher, plain and with Augment, alternating;
(c) ScenePredictor.predict with tta = 1, 4, 8 on the scene of tools/scene_bench.py, and the share of the time the two
    apply launches per op take.

    python tools/augment_bench.py [--rounds 5] [--size 4096] [--steps 20] [--out profiles/augment.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import insar_unet_ca_amd as iu  # noqa: E402
from insar_unet_ca_amd import augment as aug_mod  # noqa: E402

N, C, S = 16, 2, 256


def timed(fn, reps: int) -> float:
    """us per call: `reps` calls between two events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def torch_d4(t, op):
    b = t.transpose(-1, -2) if op & 4 else t
    dims = [d for d, bit in ((-2, 2), (-1, 1)) if op & bit]
    return torch.flip(b, dims) if dims else b


def torch_augment(x, m, ops, gain, bias, sigma):
    """What a user writes between the prefetcher and the step today: per-sample op, gain / bias broadcast, randn noise,
    masks widened to int64."""
    xo = torch.stack([torch_d4(x[s], op) for s, op in enumerate(ops)])
    xo = xo * gain.view(-1, 1, 1, 1) + bias.view(-1, 1, 1, 1)
    if sigma is not None:
        xo = xo + sigma.view(-1, 1, 1, 1) * torch.randn_like(xo)
    mo = torch.stack([torch_d4(m[s], op) for s, op in enumerate(ops)]).to(torch.int64)
    return xo.contiguous(), mo.contiguous()


def section_apply(dev, rounds: int, reps: int = 50) -> dict:
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((N, C, S, S)).astype(np.float32)).to(dev)
    m64 = torch.from_numpy(rng.integers(0, 2, size=(N, S, S)).astype(np.int64)).to(dev)
    m8 = m64.to(torch.uint8)
    out = (torch.empty_like(x), torch.empty_like(m64))
    d4_ops = [s % 8 for s in range(N)]
    cases = {"identity": ([0] * N, 0.0), "flips": ([s % 4 for s in range(N)], 0.0), "d4": (d4_ops, 0.0), "d4_noise": (d4_ops, 0.1)}
    res = {}
    for name, (ops, sg) in cases.items():
        table = torch.from_numpy(np.stack([np.asarray(ops, dtype=np.int32)] + [np.full(N, np.float32(v)).view(np.int32) for v in (1.1, 0.05, sg)], 1).copy()).to(dev)
        gain, bias = torch.full((N,), 1.1, device=dev), torch.full((N,), 0.05, device=dev)
        sigma = torch.full((N,), sg, device=dev) if sg else None
        for src_name, m in (("int64", m64), ("uint8", m8)):
            ours = lambda: aug_mod.apply_table(x, m, table, 99, out=out)
            theirs = lambda: torch_augment(x, m, ops, gain, bias, sigma)
            ours(); theirs()
            torch.cuda.synchronize()
            a, b = [], []
            for _ in range(rounds):
                a.append(timed(ours, reps))
                b.append(timed(theirs, reps))
            nbytes = x.numel() * 4 * 2 + m.numel() * (m.element_size() + 8)
            us = float(np.median(a))
            res[f"{name}/{src_name}"] = {"bytes": nbytes, "hip_us": us, "hip_us_all": a, "hip_GBps": nbytes / us / 1e3,
                                         "torch_us": float(np.median(b)), "torch_us_all": b, "torch_over_hip": float(np.median(b)) / us}
            print(f"apply {name}/{src_name}: hip {us:.1f} us ({nbytes / us / 1e3:.0f} GB/s), torch ops {np.median(b):.1f} us", flush=True)
    return res


def section_loop(dev, rounds: int, steps: int) -> dict:
    """Config 2: U-Net-CA bf16, batch 16 x 2 x 256 x 256, CrossEntropy + Adam, through DevicePrefetcher."""
    torch.manual_seed(0)
    net = iu.UNet(in_channels=C, num_classes=2, use_se=True, compute_dtype=torch.bfloat16).to(dev).train()
    crit, opt = iu.CrossEntropyLoss(ignore_index=255), iu.Adam(net.parameters(), lr=1e-4)
    rng = np.random.default_rng(1)
    batches = [(torch.from_numpy(rng.standard_normal((N, C, S, S)).astype(np.float32)).pin_memory(),
                torch.from_numpy(rng.integers(0, 2, size=(N, S, S)).astype(np.int64)).pin_memory()) for _ in range(4)]
    loader = [batches[i % 4] for i in range(steps)]

    def run(augment):
        pf = iu.DevicePrefetcher(loader, dev, augment=augment)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for xb, yb in pf:
            opt.zero_grad()
            crit(net(xb), yb).backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    aug = iu.Augment(seed=0, ops="d4", gain=(0.8, 1.25), bias=(-0.1, 0.1), noise_sigma=(0.0, 0.1))
    run(None); run(aug)                                  # warm-up of both paths
    plain, augd = [], []
    for _ in range(rounds):
        plain.append(run(None))
        augd.append(run(aug))
    print(f"loop: plain {plain} ms/step, augmented {augd} ms/step", flush=True)
    return {"steps": steps, "plain_ms_per_step": plain, "augmented_ms_per_step": augd,
            "augmented_inside_plain_spread": bool(min(plain) <= float(np.median(augd)) <= max(plain))}


def section_tta(dev, rounds: int, size: int) -> dict:
    torch.manual_seed(0)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True, compute_dtype=torch.bfloat16).to(dev).eval()
    scene = torch.from_numpy(np.random.default_rng(2).integers(0, 256, size=(size, size), dtype=np.uint8)).to(dev)
    preds = {t: iu.ScenePredictor(net, tile=256, overlap=32, batch=16, num_classes=2, tta=t) for t in (1, 4, 8)}
    times = {t: [] for t in preds}
    for t, p in preds.items():
        p.predict(scene)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for t, p in preds.items():
            t0 = time.perf_counter()
            p.predict(scene)
            torch.cuda.synchronize()
            times[t].append((time.perf_counter() - t0) * 1e3)
    # the two apply launches of one op on one batch, timed on their own
    x = torch.randn(16, 1, 256, 256, device=dev)
    lg = torch.randn(16, 2, 256, 256, device=dev)
    tab = aug_mod.constant_table([6] * 16, dev)
    xo, lo = torch.empty_like(x), torch.empty_like(lg)
    pair = lambda: (aug_mod.apply_table(x, None, tab, out=(xo, None)), aug_mod.apply_table(lg, None, tab, out=(lo, None)))
    pair()
    pair_us = float(np.median([timed(pair, 50) for _ in range(rounds)]))
    nbatches = -(-len(iu.plan_tiles(size, size, 256, 32)) // 16)
    res = {"size": size, "batches": nbatches, "apply_pair_us": pair_us}
    for t in preds:
        ms = float(np.median(times[t]))
        share = (pair_us * 1e-3 * nbatches * t / ms) if t > 1 else 0.0
        res[f"tta{t}"] = {"ms": ms, "ms_all": times[t], "apply_share": share}
        print(f"predict tta={t}: {ms:.1f} ms per scene, apply share {share:.3%}", flush=True)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sections", default="apply,loop,tta")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds}
    for name in args.sections.split(","):
        fn = {"apply": lambda: section_apply(dev, args.rounds), "loop": lambda: section_loop(dev, args.rounds, args.steps),
              "tta": lambda: section_tta(dev, args.rounds, args.size)}[name]
        result[name] = fn()
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k in ("device",)}))


if __name__ == "__main__":
    main()
