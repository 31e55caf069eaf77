"""The imbalance-aware loss entry points against the unweighted ones and against the same objectives composed from torch
ops, on one GPU: 16 x 2 x 256 x 256 fp32 logits (the loss input of the benchmarked configuration), int64 targets with a
tenth of the pixels ignored.

Legs (every round measures every leg, in turn, in one process; medians over the rounds):
  (a) insar_dice_ce                      the baseline: the fused Dice+CE objective of bench.py
  (b) insar_dice_ce_w, class weights     (c) ... weights + label smoothing     (d) ... focal (gamma 2, alpha = weights)
  (e) insar_cross_entropy_w and insar_focal against insar_cross_entropy
  (f) the same objectives written with torch ops on the device (forward + backward to the logits' gradient)
Each leg is timed by device events around `--inner` back-to-back calls; us per call, achieved GB/s on the algorithmic bytes
(fused legs: two reads of the logits, two of the targets, one write of dlogits; CE legs: one read of the logits) and the
ratio to (a). The 24 MB working set fits the 256 MiB Infinity Cache, so the GB/s figures are not bounded by HBM.

The measuring process is a child of this script, started under `timeout`; the parent never opens the device.

    python tools/loss_bench.py [--rounds 30] [--inner 20] [--out profiles/loss_weighted.json]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def child(a) -> None:
    import torch
    import torch.nn.functional as F

    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr

    if not torch.cuda.is_available():
        raise SystemExit("loss_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    B, K, H, W = a.batch, a.classes, a.size, a.size
    HW = H * W
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, K, H, W, generator=g) * 2.0).to(dev)
    target = torch.randint(0, K, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.1] = 255
    target = target.to(dev)
    weight = torch.linspace(0.2, 3.0, K).to(dev)
    nb = call("insar_ce_blocks", B * HW)
    dl = torch.empty_like(logits)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    ws = torch.empty(4 + 3 * K + nb * (3 + 3 * K), dtype=torch.float32, device=dev)     # large enough for every entry point
    st = _lib.stream_ptr
    common = (ptr(logits), ptr(target), B, K, HW, 255)
    tail = (ptr(dl), ptr(out), ptr(ws))

    def dice_ce():
        call("insar_dice_ce", *common, 1.0, 1.0, 1.0, *tail, st())

    def dice_ce_w(eps, gamma):
        return lambda: call("insar_dice_ce_w", *common, 1.0, 1.0, 1.0, ptr(weight), eps, gamma, *tail, st())

    def ce():
        call("insar_cross_entropy", *common, *tail, st())

    def ce_w(eps):
        return lambda: call("insar_cross_entropy_w", *common, ptr(weight), eps, *tail, st())

    def focal():
        call("insar_focal", *common, 2.0, ptr(weight), *tail, st())

    # ---- the torch-op alternative: forward + backward to d loss / d logits ---------------------------------------------
    lg_t = logits.clone().requires_grad_(True)
    valid = target != 255
    safe = torch.where(valid, target, torch.zeros_like(target))
    onehot = F.one_hot(safe, K).permute(0, 3, 1, 2).float() * valid.unsqueeze(1)

    def t_dice(x):
        p = torch.softmax(x, 1) * valid.unsqueeze(1)
        inter = (p * onehot).sum(dim=(0, 2, 3))
        den = p.sum(dim=(0, 2, 3)) + onehot.sum(dim=(0, 2, 3))
        return 1.0 - ((2 * inter + 1.0) / (den + 1.0)).mean()

    def t_focal(x):
        lp = torch.log_softmax(x, 1).gather(1, safe.unsqueeze(1)).squeeze(1)
        return (weight[safe] * (1.0 - lp.exp()).pow(2.0) * (-lp) * valid).sum() / valid.sum()

    def torch_leg(fn):
        def run():
            lg_t.grad = None
            fn(lg_t).backward()
        return run

    legs = {
        "a_dice_ce": (dice_ce, "fused"),
        "b_dice_ce_w_weights": (dice_ce_w(0.0, -1.0), "fused"),
        "c_dice_ce_w_weights_smoothing": (dice_ce_w(0.1, -1.0), "fused"),
        "d_dice_ce_w_focal": (dice_ce_w(0.0, 2.0), "fused"),
        "e_cross_entropy": (ce, "ce"),
        "e_cross_entropy_w": (ce_w(0.0), "ce"),
        "e_cross_entropy_w_smoothing": (ce_w(0.1), "ce"),
        "e_focal": (focal, "ce"),
        "f_torch_dice_ce": (torch_leg(lambda x: F.cross_entropy(x, target, ignore_index=255) + t_dice(x)), "fused"),
        "f_torch_dice_ce_weights": (torch_leg(lambda x: F.cross_entropy(x, target, weight=weight, ignore_index=255) + t_dice(x)), "fused"),
        "f_torch_dice_ce_weights_smoothing": (torch_leg(lambda x: F.cross_entropy(x, target, weight=weight, ignore_index=255,
                                                                                  label_smoothing=0.1) + t_dice(x)), "fused"),
        "f_torch_dice_focal": (torch_leg(lambda x: t_focal(x) + t_dice(x)), "fused"),
        "f_torch_cross_entropy_weights": (torch_leg(lambda x: F.cross_entropy(x, target, weight=weight, ignore_index=255)), "ce"),
    }
    lbytes, tbytes = logits.numel() * 4, target.numel() * 8
    nbytes = {"fused": 2 * lbytes + 2 * tbytes + lbytes, "ce": lbytes + 2 * tbytes + lbytes}

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / inner          # us per call

    for fn, _ in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    # agreement of the new fused entry point with the baseline where they compute the same thing (weights = null, eps = 0)
    dice_ce()
    ref_out, ref_dl = out.clone(), dl.clone()
    call("insar_dice_ce_w", *common, 1.0, 1.0, 1.0, 0, 0.0, -1.0, *tail, st())
    agree = {"loss_abs_diff": float((out[0] - ref_out[0]).abs()), "dlogits_max_abs_diff": float((dl - ref_dl).abs().max())}

    t = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, (fn, _) in legs.items():
            t[k].append(timed(fn, a.inner))
    base = median(t["a_dice_ce"])
    res = {}
    for k, (_, kind) in legs.items():
        us = median(t[k])
        res[k] = {"us_per_call": round(us, 3), "min_us": round(min(t[k]), 3), "max_us": round(max(t[k]), 3),
                  "algorithmic_bytes": nbytes[kind], "GBps": round(nbytes[kind] / (us * 1e-6) / 1e9, 1),
                  "ratio_to_a": round(us / base, 4)}
    res["e_cross_entropy_w"]["ratio_to_cross_entropy"] = round(res["e_cross_entropy_w"]["us_per_call"] / res["e_cross_entropy"]["us_per_call"], 4)
    res["e_focal"]["ratio_to_cross_entropy"] = round(res["e_focal"]["us_per_call"] / res["e_cross_entropy"]["us_per_call"], 4)
    doc = {"logits": [B, K, H, W], "dtype": "float32", "ignored_fraction": 0.1, "rounds": a.rounds, "inner_calls_per_event_pair": a.inner,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "timing": "device events, median over rounds, legs interleaved",
           "note": "24 MB working set: resident in the 256 MiB Infinity Cache, GB/s is not an HBM figure",
           "weighted_vs_baseline_with_null_weights": agree, "legs": res}
    line = json.dumps(doc)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        raise SystemExit(f"loss_bench: the measuring process ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
