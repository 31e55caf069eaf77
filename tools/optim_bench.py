"""AdamW (csrc/optim_w.hip) against the Adam launch of the benchmarked step and against the same recipe in torch ops, on one
GPU: the 31.26 M parameters of U-Net-CA in the model's own tensor shapes, fp32, gradients shared by every leg.

Legs (every round measures every leg, in turn, in one process; medians over the rounds), us per optimizer step:
  (a) insar_adam_step_dev                                  the baseline: what bench.py's step runs (not touched by AdamW)
  (b) AdamW plain (weight_decay = 0)   (c) + decay, two groups (split_decay_groups)   (d) + clip   (e) + EMA   (f) all together
      with a poly schedule: the C entry points launched from the optimizer's own cached tables (AdamW._launch)
  (g) AdamW.step() of (f) through Python: the same launches plus the steady-state pointer check over the parameters
  (h) torch.optim.AdamW(foreach=True) on the two groups + clip_grad_norm_ + a foreach EMA (lerp)
Each leg is timed by device events around `--inner` back-to-back steps; beside the time: the byte model (28 B per parameter;
+4 norm pass, +8 EMA), the time that model takes at the HBM rate BASELINE.md measured (6.29 TB/s), and the ratio to (a).
The 125 MB of gradients are read cold here; in a training step they may still sit in the 256 MiB Infinity Cache right after
backward, which this stand-alone tool does not reproduce.

The measuring process is a child of this script, started under `timeout`; the parent never opens the device.

    python tools/optim_bench.py [--rounds 30] [--inner 10] [--out profiles/optim_adamw.json]
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

HBM_BPS = 6.29e12      # measured copy rate of one MI355X


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def child(a) -> None:
    import torch

    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib, optim
    from insar_unet_ca_amd._lib import call, ptr

    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    shapes = [tuple(p.shape) for p in iu.UNet(2, 2, True).parameters()]
    nparam = sum(int(torch.Size(s).numel()) for s in shapes)
    g = torch.Generator().manual_seed(0)
    grads = [(torch.randn(s, generator=g) * 1e-2).to(dev) for s in shapes]
    init = [(torch.randn(s, generator=g) * 0.1) for s in shapes]

    def params():
        ps = [torch.nn.Parameter(t.to(dev)) for t in init]
        for p, gr in zip(ps, grads):
            p.grad = gr
        return ps

    def groups(ps):
        return [{"params": [p for p in ps if p.ndim > 1], "weight_decay": 1e-2}, {"params": [p for p in ps if p.ndim <= 1], "weight_decay": 0.0}]

    sched = iu.LRSchedule("poly", 100000, warmup_steps=500, warmup_start=0.01)
    adam = iu.Adam(params(), lr=1e-4)
    adam.enable_device_step()
    adam.step(); adam.step()
    _, _, _, table, chunk_t, nchunks, _ = adam._fast

    def adam_dev():
        call("insar_adam_step_dev", ptr(table), ptr(chunk_t), nchunks, optim.CHUNK, 1e-4, 0.9, 0.999, 1e-8, ptr(adam._dev_state), 1.0,
             _lib.stream_ptr())

    def adamw(grouped, **kw):
        ps = params()
        opt = iu.AdamW(groups(ps) if grouped else ps, lr=1e-4, weight_decay=1e-2 if grouped else 0.0, **kw)
        opt.step(); opt.step()
        launch = opt._fast[4]
        return opt, (lambda: opt._launch(*launch))

    o_plain, f_plain = adamw(False)
    o_decay, f_decay = adamw(True)
    o_clip, f_clip = adamw(True, max_grad_norm=1.0)
    o_ema, f_ema = adamw(True, ema_decay=0.999)
    o_all, f_all = adamw(True, max_grad_norm=1.0, ema_decay=0.999, schedule=sched, skip_nonfinite=True)

    tps = params()
    topt = torch.optim.AdamW(groups(tps), lr=1e-4, foreach=True)
    tema = [p.detach().clone() for p in tps]

    def torch_recipe():
        torch.nn.utils.clip_grad_norm_(tps, 1.0, foreach=True)       # scales the shared gradients only when the norm exceeds 1
        topt.step()
        with torch.no_grad():
            torch._foreach_lerp_(tema, [p.detach() for p in tps], 1e-3)

    B = 4 * nparam
    legs = {
        "a_insar_adam_step_dev": (adam_dev, 7 * B),
        "b_adamw_plain": (f_plain, 7 * B),
        "c_adamw_decay_groups": (f_decay, 7 * B),
        "d_adamw_decay_clip": (f_clip, 8 * B),
        "e_adamw_decay_ema": (f_ema, 9 * B),
        "f_adamw_all": (f_all, 10 * B),
        "g_adamw_all_python_step": (o_all.step, 10 * B),
        "h_torch_foreach_adamw_clip_ema": (torch_recipe, None),
    }

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / inner          # us per step

    for fn, _ in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, (fn, _) in legs.items():
            t[k].append(timed(fn, a.inner))
    base = median(t["a_insar_adam_step_dev"])
    res = {}
    for k, (_, nbytes) in legs.items():
        us = median(t[k])
        res[k] = {"us_per_step": round(us, 2), "min_us": round(min(t[k]), 2), "max_us": round(max(t[k]), 2), "ratio_to_a": round(us / base, 4)}
        if nbytes:
            res[k].update(bytes_per_param=nbytes // nparam, model_us_at_hbm_rate=round(nbytes / HBM_BPS * 1e6, 2),
                          TBps=round(nbytes / (us * 1e-6) / 1e12, 3))
    state = o_all._read_state()
    doc = {"parameters": nparam, "tensors": len(shapes), "chunks": nchunks, "dtype": "float32", "rounds": a.rounds,
           "inner_steps_per_event_pair": a.inner, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "timing": "device events, median over rounds, legs interleaved", "hbm_rate_TBps": HBM_BPS / 1e12,
           "note": "gradients are read cold (stand-alone): in a training step they may still sit in the Infinity Cache after backward",
           "all_leg_state_after": {"t": state["t"], "skipped": state["skipped"], "grad_norm": state["grad_norm"], "coef": state["coef"]},
           "legs": res}
    line = json.dumps(doc)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
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
        raise SystemExit(f"optim_bench: the measuring process ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
