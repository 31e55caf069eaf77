"""The tensor set and configurations of tests/test_adamw_gpu.py, and the float32 floor from which its tolerance factors
come. Everything here is host arithmetic on fixed-seed values.

Tensor set: the smallest that reaches every path of csrc/optim_w.hip at chunk size 8192: a single element, sizes below /
at / above one float4, one chunk minus / exactly / plus one element, three chunks with a partial last one; tensor 4 (8191
elements) starts 4 bytes into its buffer (parameter and gradient: the element-wise paths of both kernels), tensors 3 and
6 are 16-byte aligned with numel % 4 == 1 (float4 body + element-wise tail)."""
from __future__ import annotations

import numpy as np

from tests import optim_ref as ref

SIZES = (1, 3, 4, 5, 8191, 8192, 8193, 20000)
UNALIGNED = 4
STEPS = 3
BASE_LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
BETAS_F32 = tuple(float(np.float32(b)) for b in BETAS)      # what the update kernel receives
SCHEDULE = dict(kind="poly", total_steps=12, warmup_steps=3, warmup_start=0.1, min_lr=1e-4, power=0.9)
EPS24 = 2.0 ** -24


def make_values(seed: int = 1234, steps: int = STEPS):
    """(parameters, [gradients of step 1, 2, ...]) as float32 arrays. Some gradient elements are exactly zero (v stays 0 there
    on the first step) and the scale changes from step to step."""
    rng = np.random.default_rng(seed)
    params = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
    grads = []
    for s in range(steps):
        gs = [((0.02, 3.0, 0.4)[s % 3] * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
        for g in gs:
            g[::97] = 0.0 if g.size > 97 else g[::97]
        grads.append(gs)
    return params, grads


def group_of(i: int) -> int:
    """The "groups" configuration: even tensors decay at the base rate, odd ones are exempt and run at a quarter of it."""
    return i % 2


# name -> AdamW keyword arguments (max_grad_norm "half": half the norm of the first step's scaled gradients)
CONFIGS = {
    "decoupled": dict(weight_decay=0.1),
    "l2": dict(weight_decay=0.1, decoupled=False),
    "groups": dict(weight_decay=0.1, groups=True),
    "clip": dict(weight_decay=0.0, max_grad_norm="half"),
    "ema": dict(weight_decay=0.0, ema_decay=0.9),
    "all": dict(weight_decay=0.1, groups=True, max_grad_norm="half", ema_decay=0.9, schedule=True, grad_scale=0.25),
}


def resolve(name: str, grads):
    """Configuration with the clip bound turned into a number."""
    cfg = dict(decoupled=True, groups=False, max_grad_norm=None, ema_decay=None, schedule=False, grad_scale=1.0)
    cfg.update(CONFIGS[name])
    if cfg["max_grad_norm"] == "half":
        cfg["max_grad_norm"] = 0.5 * ref.grad_norm(grads[0], cfg["grad_scale"])
    return cfg


def reference_step(cfg, t, state, grads, dtype=np.float64, coef=None):
    """Step t of every tensor from `state` = [(p, m, v, ema or None)] (float32 values): (norm, coef, lr, outputs, units).
    coef: the clip coefficient the update launch actually read (a float32 in the state block, judged on its own against the
    norm's bound); None: the reference's own."""
    gs = cfg["grad_scale"]
    norm = ref.grad_norm(grads, gs, dtype) if cfg["max_grad_norm"] is not None else None
    if coef is None:
        coef = ref.clip_coef(norm, cfg["max_grad_norm"]) if norm is not None else 1.0
    lr = ref.lr_at(base_lr=BASE_LR, t=t - 1, **SCHEDULE) if cfg["schedule"] else BASE_LR
    alpha = None if cfg["ema_decay"] is None else 1.0 - ref.ema_decay_at(cfg["ema_decay"], t)
    outs, units = [], []
    for i, ((p, m, v, e), g) in enumerate(zip(state, grads)):
        exempt = cfg["groups"] and group_of(i) == 1
        o, u = ref.step(p, g, m, v, e, t, lr=lr, betas=BETAS, eps=EPS, weight_decay=0.0 if exempt else cfg["weight_decay"],
                        decoupled=cfg["decoupled"], grad_scale=gs, coef=coef, lr_mult=0.25 if exempt else 1.0, ema_alpha=alpha, update_betas=BETAS_F32,
                        dtype=dtype)
        outs.append(o)
        units.append(u)
    return norm, coef, lr, outs, units


def ratios(got, want, units):
    """Largest |got - want| / (2^-24 U) per output kind (p, m, v, ema) over the tensors of one step."""
    worst = [0.0, 0.0, 0.0, 0.0]
    for g, w, u in zip(got, want, units):
        for k in range(4):
            if w[k] is None:
                continue
            err = np.abs(np.asarray(g[k], np.float64) - w[k])
            den = EPS24 * u[k]
            assert np.all(err[den == 0] == 0)
            worst[k] = max(worst[k], float((err[den > 0] / den[den > 0]).max(initial=0.0)))
    return worst


def float32_floor():
    """The reference's own formulas in float32 (every operation rounded, strictly sequential sums) against float64, on the
    cases of the GPU test, each step starting from the float32 state the float32 evaluation left: the largest ratio per
    output kind, and for the norm."""
    params, grads = make_values()
    worst, worst_norm = [0.0] * 4, 0.0
    for name in CONFIGS:
        cfg = resolve(name, grads)
        state = [(p, np.zeros_like(p), np.zeros_like(p), p.copy() if cfg["ema_decay"] is not None else None) for p in params]
        for t in range(1, STEPS + 1):
            n32, c32, _, got, _ = reference_step(cfg, t, state, grads[t - 1], np.float32)
            n64, _, _, want, units = reference_step(cfg, t, state, grads[t - 1], coef=float(np.float32(c32)))
            worst = [max(a, b) for a, b in zip(worst, ratios(got, want, units))]
            if n64 is not None:
                worst_norm = max(worst_norm, abs(n32 - n64) / (EPS24 * ref.norm_unit(grads[t - 1], cfg["grad_scale"])[2]))
            state = [tuple(None if x is None else np.asarray(x, np.float32) for x in o) for o in got]
    return dict(zip(("p", "m", "v", "ema"), worst), norm=worst_norm)


# k = 2 x the floor above (tests/test_adamw_host.py checks these against float32_floor()), fixed before a kernel ran
K = {"p": 1.842, "m": 1.829, "v": 1.907, "ema": 0.929, "norm": 1.622}
