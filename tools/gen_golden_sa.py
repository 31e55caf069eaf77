"""Fixtures of the SA U-Net (Unet-SpatialAttention.py) from the reference script itself, on CPU:

  tests/golden/g11_sa_block.npz        SpatialAttention block cases: output, input gradient, the 10 parameter gradients and
                                       the BatchNorm buffers after each of two training steps (C = 128, 1024; train / eval;
                                       one input with exact channel-max ties)
  tests/golden/g11_sa_block_full.npz   the C = 1024 cases' step-0 output and input gradient, whole
  tests/golden/g11_unet_sa.npz         2 x 2 x 64 x 64 fp32 network: train / eval logits, per-tensor gradient norms,
                                       a 5-step Adam loss trajectory
  tests/golden/g11_unet_sa_contract.json  state_dict keys, shapes, order and parameter count (in_channels = 2)

Every value is computed twice, in float32 and float64; the float64 result is stored and `<key>/noise` holds torch's own
float32-vs-float64 deviation (max |f32 - f64| / max |f64|), so the tests' tolerances are multiples of the reference's own
rounding noise. Weights and inputs come from oracle.closed_form (numpy PCG64 / closed-form sines: no torch RNG).

    python tools/gen_golden_sa.py          (needs the reference tree; writes the three files)
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import closed_form as cf  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SCRIPT = "Unet-SpatialAttention.py"
FULL_LIMIT = 16384
NSAMPLE = 64

# (tag, shape, training, input kind)
BLOCK_CASES = (("c128_train", (2, 128, 8, 8), True, "sep"),
               ("c128_eval", (2, 128, 8, 8), False, "sep"),
               ("c1024_train", (2, 1024, 4, 4), True, "sep"),
               ("c1024_eval", (2, 1024, 4, 4), False, "sep"),
               ("ties_train", (2, 64, 8, 8), True, "ties"))
NET_SHAPE = (2, 2, 64, 64)
ADAM_STEPS, ADAM_LR = 5, 1e-4


def available() -> bool:
    return os.path.isfile(os.path.join(ref_loader.REFERENCE_ROOT, SCRIPT))


def load_reference():
    ref_loader._install_torchvision_stub()
    spec = importlib.util.spec_from_file_location("ref_unet_sa", os.path.join(ref_loader.REFERENCE_ROOT, SCRIPT))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def block_input(shape, kind: str) -> torch.Tensor:
    """'sep': generic values with one channel per pixel lifted by 2 (separated maxima: the arg-max is the same in fp32 and
    bf16); 'ties': values on a 1/4 grid (exact in bf16), the maximum held by several channels at most pixels."""
    b, c, h, w = shape
    if kind == "ties":
        x = cf.make_input(shape, 0.3)
        return (torch.round(x * 4.0) / 4.0).contiguous()
    x = cf.make_input_random(shape, seed=21 + c)
    pix = np.arange(b * h * w).reshape(b, h, w)
    top = torch.from_numpy((pix * 7919 + 13) % c)
    x.scatter_add_(1, top.unsqueeze(1), torch.full((b, 1, h, w), 2.0))
    return x


def block_grad(shape) -> torch.Tensor:
    return cf.make_input_random(shape, seed=5)


def sa_state(mod_sa, seed: int = 3):
    return cf.fill_state_dict_random(mod_sa.state_dict(), seed=seed)


def _summ(prefix: str, a64: torch.Tensor, a32: torch.Tensor, store: dict) -> None:
    a = a64.detach().double().reshape(-1).numpy()
    b = a32.detach().double().reshape(-1).numpy()
    store[f"{prefix}/norm"] = np.array(np.sqrt((a * a).sum()))
    store[f"{prefix}/sum"] = np.array(a.sum())
    store[f"{prefix}/absmax"] = np.array(np.abs(a).max() if a.size else 0.0)
    store[f"{prefix}/samples"] = a[cf.sample_indices(a.size, NSAMPLE)].astype(np.float32)
    den = np.abs(a).max()
    store[f"{prefix}/noise"] = np.array(np.abs(a - b).max() / den if den > 0 else np.abs(b).max())
    if a.size <= FULL_LIMIT:
        store[f"{prefix}/full"] = a64.detach().float().numpy().reshape(a64.shape).copy()


def block_run(ref, shape, training: bool, kind: str, dtype):
    sa = ref.SpatialAttention()
    sa.load_state_dict(sa_state(sa))
    sa = sa.to(dtype).train(training)
    x0, g = block_input(shape, kind).to(dtype), block_grad(shape).to(dtype)
    steps = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        for p in sa.parameters():
            p.grad = None
        out = sa(x)
        out.backward(g)
        steps.append({"out": out.detach().clone(), "dx": x.grad.clone(),
                      **{f"grad/{k}": p.grad.clone() for k, p in sa.named_parameters()},
                      **{f"buf/{k}": b.clone() for k, b in sa.named_buffers() if not k.endswith("num_batches_tracked")}})
    return steps


def gen_block(ref):
    """(g11_sa_block, g11_sa_block_full): the second holds the step-0 output and input gradient of the cases whose tensors
    are too large for FULL_LIMIT (C = 1024), whole, so that every element of them is checked."""
    store, full = {}, {}
    for tag, shape, training, kind in BLOCK_CASES:
        r64 = block_run(ref, shape, training, kind, torch.float64)
        r32 = block_run(ref, shape, training, kind, torch.float32)
        for s in range(2):
            for k in r64[s]:
                _summ(f"{tag}/step{s}/{k}", r64[s][k], r32[s][k], store)
        for k in ("out", "dx"):
            if r64[0][k].numel() > FULL_LIMIT:
                full[f"{tag}/step0/{k}/full"] = r64[0][k].float().numpy().copy()
        store[f"{tag}/shape"] = np.array(shape)
        store[f"{tag}/training"] = np.array(int(training))
    return store, full


def net_setup(ref, dtype):
    net = ref.UNet(in_channels=2, num_classes=2)
    net.load_state_dict(cf.fill_state_dict_random(net.state_dict(), seed=7))
    return net.to(dtype)


def net_inputs():
    return (cf.make_input_random(NET_SHAPE, seed=11),
            cf.make_target_random((NET_SHAPE[0],) + NET_SHAPE[2:], seed=13, ignore_frac=0.05))


def net_run(ref, dtype) -> dict:
    x, tgt = net_inputs()
    x = x.to(dtype)
    crit = nn.CrossEntropyLoss(ignore_index=255)
    out = {}
    net = net_setup(ref, dtype).train()
    logits = net(x)
    loss = crit(logits, tgt)
    loss.backward()
    out["train/logits"] = logits.detach().clone()
    out["train/loss"] = loss.detach().reshape(1)
    for k, p in net.named_parameters():
        out[f"train/gradnorm/{k}"] = p.grad.detach().norm().reshape(1)
    net_e = net_setup(ref, dtype).eval()
    with torch.no_grad():
        out["eval/logits"] = net_e(x).clone()
    net_a = net_setup(ref, dtype).train()
    opt = torch.optim.Adam(net_a.parameters(), lr=ADAM_LR)
    losses = []
    for _ in range(ADAM_STEPS):
        opt.zero_grad()
        l = crit(net_a(x), tgt)
        l.backward()
        opt.step()
        losses.append(l.detach().reshape(1))
    out["adam/loss"] = torch.cat(losses)
    return out


def gen_net(ref) -> dict:
    r64, r32 = net_run(ref, torch.float64), net_run(ref, torch.float32)
    store = {}
    for k in r64:
        _summ(k, r64[k], r32[k], store)
    return store


def gen_contract(ref) -> dict:
    sd = ref.UNet(in_channels=2, num_classes=2).state_dict()
    net = ref.UNet(in_channels=2, num_classes=2)
    return {"in_channels": 2, "num_classes": 2, "entries": len(sd),
            "parameters": int(sum(p.numel() for p in net.parameters())),
            "keys": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()]}


def generate() -> dict:
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    ref = load_reference()
    block, block_full = gen_block(ref)
    return {"g11_sa_block": block, "g11_sa_block_full": block_full, "g11_unet_sa": gen_net(ref),
            "g11_unet_sa_contract": gen_contract(ref)}


def main() -> None:
    if not available():
        raise SystemExit(f"{SCRIPT} not found under {ref_loader.REFERENCE_ROOT}")
    out = generate()
    np.savez_compressed(os.path.join(OUT, "g11_sa_block.npz"), **out["g11_sa_block"])
    np.savez_compressed(os.path.join(OUT, "g11_sa_block_full.npz"), **out["g11_sa_block_full"])
    np.savez_compressed(os.path.join(OUT, "g11_unet_sa.npz"), **out["g11_unet_sa"])
    with open(os.path.join(OUT, "g11_unet_sa_contract.json"), "w") as f:
        json.dump(out["g11_unet_sa_contract"], f, indent=0)
        f.write("\n")
    for name in ("g11_sa_block.npz", "g11_sa_block_full.npz", "g11_unet_sa.npz", "g11_unet_sa_contract.json"):
        print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")


if __name__ == "__main__":
    main()
