"""Reference for insar_unet_ca_amd.AdamW: one step from given (p, g, m, v, ema, t) in plain formulas. It restates the
specification (include/insar_hip.h, "AdamW, clipping, schedule, EMA" in DESIGN.md) and does not read the kernels;
tests/test_adamw_host.py pins it to torch.optim.AdamW / Adam(weight_decay=) / clip_grad_norm_ / LambdaLR in float64.

`dtype=np.float32` evaluates the SAME formulas with every operation rounded to float32 (strictly sequential sums): the floor
from which the GPU test's tolerance factor k is taken. Next to each output the step returns its running error unit U: the
magnitudes of everything that gets rounded on the way to it, carried through the chain, so that a float32 evaluation is
expected within a small multiple of 2^-24 * U."""
from __future__ import annotations

import math

import numpy as np


def lr_at(kind, base_lr, t, total_steps=0, warmup_steps=0, warmup_start=0.0, min_lr=0.0, power=0.9):
    """Learning rate of the step taken after t finished steps (kind None: no schedule)."""
    if kind is None:
        return base_lr
    if t < warmup_steps:
        return base_lr * (warmup_start + (1.0 - warmup_start) * (t / warmup_steps))
    if kind == "constant":
        return base_lr
    if t >= total_steps:
        return min_lr
    q = (t - warmup_steps) / (total_steps - warmup_steps)
    if kind == "cosine":
        return min_lr + (base_lr - min_lr) * (0.5 * (1.0 + math.cos(math.pi * q)))
    if kind == "poly":
        return min_lr + (base_lr - min_lr) * (1.0 - q) ** power
    raise ValueError(kind)


def ema_decay_at(decay, t, warmup=True):
    """decay_t of step t (t counts from 1)."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def sum_squares(grads, grad_scale=1.0, dtype=np.float64):
    """sum (g * grad_scale)^2 over every tensor; float32: one strictly sequential running sum."""
    if dtype == np.float64:
        return float(sum(((np.asarray(g, np.float64) * grad_scale) ** 2).sum() for g in grads))
    acc, gs = np.float32(0), np.float32(grad_scale)
    for g in grads:
        x = np.asarray(g, np.float32).ravel() * gs
        acc = np.cumsum(np.concatenate([[acc], x * x]).astype(np.float32), dtype=np.float32)[-1]
    return float(acc)


def grad_norm(grads, grad_scale=1.0, dtype=np.float64):
    return math.sqrt(sum_squares(grads, grad_scale, dtype))


def norm_unit(grads, grad_scale=1.0):
    """(n, S, U of the norm): a sum of n terms has U = sqrt(n) * S; through the square root, plus the norm's own rounding."""
    n = sum(int(np.asarray(g).size) for g in grads)
    S = sum_squares(grads, grad_scale)
    nrm = math.sqrt(S)
    return n, S, (math.sqrt(n) * S / (2.0 * nrm) + nrm if nrm > 0 else 0.0)


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)); None: no clipping."""
    if max_norm is None:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def step(p, g, m, v, ema, t, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, grad_scale=1.0, coef=1.0,
         lr_mult=1.0, ema_alpha=None, update_betas=None, dtype=np.float64):
    """Step number t (>= 1) of one tensor. lr: the base rate of this step (schedule already applied). Returns
    (p, m, v, ema) and their error units (Up, Um, Uv, Ue); ema / Ue are None without an EMA.
    update_betas: the betas of the two moment recurrences where they differ from those of the bias corrections: the C ABI
    takes beta1 / beta2 of the update as float (as insar_adam_step does) and those of the corrections as double, so against
    the kernels the recurrences run on float32(beta)."""
    f = dtype
    b1, b2 = betas
    u1, u2 = update_betas or betas
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    # scalars the kernel receives or reads as float32
    lr_s, bc1, bc2s = f(f(lr) * f(lr_mult)), f(1.0 - b1 ** t), f(math.sqrt(1.0 - b2 ** t))
    s, wd, omb1, omb2, b2f, epsf = f(f(grad_scale) * f(coef)), f(weight_decay), f(1) - f(u1), f(1) - f(u2), f(u2), f(eps)
    gj = g * s
    ug = 2.0 * np.abs(gj)
    if decoupled:
        cw = f(lr_s * wd)
        p1 = p - cw * p
        up1 = np.abs(p) + 4.0 * np.abs(cw * p)
    else:
        gj = gj + wd * p
        ug = ug + 2.0 * np.abs(wd * p) + np.abs(gj)
        p1, up1 = p, 0.0 * np.abs(p)
    m2 = m + (gj - m) * omb1
    um = np.abs(m) + np.abs(gj) + ug
    v2 = v * b2f + omb2 * gj * gj
    uv = np.abs(v * b2f) + 3.0 * omb2 * gj * gj + 2.0 * omb2 * np.abs(gj) * ug + np.abs(v2)
    root = np.sqrt(v2)
    den = root / bc2s + epsf
    safe = np.where(root > 0, root, 1.0)
    uden = (uv / (2.0 * safe) + 2.0 * root) / bc2s + np.abs(den)
    q = m2 / den
    uq = um / den + np.abs(m2) * uden / (den * den) + np.abs(q)
    c = f(lr_s / bc1)
    upd = c * q
    p2 = p1 - upd
    up = up1 + 5.0 * np.abs(upd) + np.abs(c) * uq + np.abs(p2)
    e2 = ue = None
    if ema_alpha is not None:
        a = f(ema_alpha)
        e = np.asarray(ema, f)
        e2 = e + (p2 - e) * a
        ue = np.abs(e) + a * (np.abs(p2) + np.abs(e) + up) + 2.0 * np.abs((p2 - e) * a) + np.abs(e2)
    as64 = lambda x: None if x is None else np.asarray(x, np.float64)
    return (p2, m2, v2, e2), tuple(as64(u) for u in (up, um, uv, ue))
