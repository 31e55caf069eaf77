"""Step time of FCN-SE, FCN and DeepLabV3-CA on the same box, in one process: bf16, 16 x 1 x 256 x 256 (config 5's
geometry), zero_grad -> forward -> CE -> backward -> Adam, device-synchronised per timed window. Also the launches of one
steady-state step (eager launch sequence through the C-ABI wrapper, geometry queries excluded). Rounds interleave the three models.

    python tools/fcn_bench.py [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/fcn_bench.json]
    python tools/fcn_bench.py --only FCN_SingleChannel_SE --steps 10     (one model, e.g. under rocprofv3)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import insar_unet_ca_amd as iu  # noqa: E402
from insar_unet_ca_amd import _lib  # noqa: E402
from insar_unet_ca_amd.data import make_batch  # noqa: E402

MODELS = ("FCN_SingleChannel_SE", "FCN_SingleChannel", "DeepLabV3_SingleChannel_Attn")


def build(name, dev):
    torch.manual_seed(0)
    net = getattr(iu, name)(num_classes=2, backbone="resnet50", pretrained=False, compute_dtype=torch.bfloat16)
    net = net.to(dev).train()
    return net, iu.CrossEntropyLoss(ignore_index=255), iu.Adam(net.parameters(), lr=1e-4)


def step(net, crit, opt, x, y):
    opt.zero_grad()
    loss = crit(net(x), y)
    loss.backward()
    opt.step()
    return loss


def count_launches(net, crit, opt, x, y) -> int:
    from insar_unet_ca_amd import tape
    old_mode, old_call = tape.MODE, _lib.call
    n = [0]

    def counting(name, *a):
        if name not in _lib._COUNT_ONLY:             # launches only: the geometry queries are host arithmetic
            n[0] += 1
        return old_call(name, *a)
    mods = [m for k, m in sys.modules.items() if k.startswith("insar_unet_ca_amd") and getattr(m, "call", None) is old_call]
    tape.MODE = "0"
    try:
        for m in mods:
            m.call = counting
        _lib.call = counting
        step(net, crit, opt, x, y)
        torch.cuda.synchronize()
    finally:
        for m in mods:
            m.call = old_call
        _lib.call = old_call
        tape.MODE = old_mode
    return n[0]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x, y = (t.to(dev) for t in make_batch(0, 16, 256, channels=1))
    names = [a.only] if a.only else list(MODELS)
    runs = {n: build(n, dev) for n in names}
    for n in names:
        for _ in range(a.warmup):
            step(*runs[n], x, y)
    torch.cuda.synchronize()
    # launches of one steady-state step (plans built, weights laid out), counted on the eager launch sequence
    res = {n: {"ms_per_step": [], "launches_per_step": count_launches(*runs[n], x, y)} for n in names}
    for n in names:
        step(*runs[n], x, y)                         # back to the launch tapes before the timed rounds
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for n in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step(*runs[n], x, y)
            torch.cuda.synchronize()
            res[n]["ms_per_step"].append((time.perf_counter() - t0) * 1e3 / a.steps)
            res[n]["loss"] = float(loss)
    for n in names:
        v = sorted(res[n]["ms_per_step"])
        res[n]["ms_per_step_median"] = v[len(v) // 2]
    out = {"geometry": [16, 1, 256, 256], "dtype": "bfloat16", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "results": res}
    if "FCN_SingleChannel_SE" in res and "FCN_SingleChannel" in res:
        out["se_overhead_ms"] = res["FCN_SingleChannel_SE"]["ms_per_step_median"] - res["FCN_SingleChannel"]["ms_per_step_median"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
