"""Fixtures of the two FCN scripts (PSPNet.py, PSPNet-ChannelAttention.py), from the reference's own code on CPU:

  tests/golden/g12_fcn_contract.json   for FCN_SingleChannel and FCN_SingleChannel_SE (num_classes = 2): keys in order,
                                       shapes, dtypes, entry and parameter counts, and per-tensor fingerprints (sum, sum of
                                       squares, three fixed elements) of the seed-0 initialisation, which pin the order in
                                       which the constructors consume torch's RNG.
  tests/golden/g12_se_bottleneck.npz   the reference's BottleneckWithSE around four blocks of its FCN-SE (layer1.0 with its
                                       downsample, layer2.0 stride 2, layer3.1 dilation 2, layer4.1 C = 2048 dilation 4), train
                                       and eval mode, two steps each: output, input gradient, every parameter gradient and the
                                       BatchNorm buffers after the step.
  tests/golden/g12_fcn.npz             FCN-SE and FCN at 2 x 1 x 64 x 64 (dropout p = 0): train / eval logits, the loss,
                                       per-tensor gradient norms and a 5-step Adam(1e-4) loss trajectory.

Every value of the two npz files is computed in float32 and float64: the float64 result is stored and `<key>/noise` holds
torch's own float32-vs-float64 deviation (max |f32 - f64| / max |f64|); tensors are stored as norm, sum, absmax, 64 fixed
samples (and whole when small). Weights and inputs come from oracle.closed_form (numpy PCG64: no torch RNG).

torchvision is not installed, so a stub provides what the scripts import from it: `models.resnet.Bottleneck` and
`models.segmentation.fcn_resnet50` / `fcn.FCNHead` restated (insar_unet_ca_amd.deeplab / .fcn: the published module
structure, unpinned like DeepLabV3's). With it, the reference's own constructors, SEBlock and BottleneckWithSE run.

    python tools/gen_golden_fcn.py          (needs the reference tree; writes the three files)
"""
from __future__ import annotations

import copy
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import closed_form as cf  # noqa: E402
from oracle import ref_loader  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "g12_fcn_contract.json")
FULL_LIMIT = 4096
NSAMPLE = 64
# (tag, layer, block index, input shape): the block's input is (B, C_in, H, W)
BLOCK_CASES = (("l1b0", "layer1", 0, (2, 64, 8, 8)), ("l2b0", "layer2", 0, (2, 256, 8, 8)),
               ("l3b1", "layer3", 1, (2, 1024, 8, 8)), ("l4b1", "layer4", 1, (2, 2048, 8, 8)))
BLOCK_SEED, BLOCK_X_SEED, BLOCK_G_SEED = 3, 21, 5
NET_SHAPE, NET_SEED, NET_X_SEED, NET_T_SEED = (2, 1, 64, 64), 7, 11, 13
ADAM_STEPS, ADAM_LR = 5, 1e-4
SCRIPTS = {"FCN_SingleChannel": "PSPNet.py", "FCN_SingleChannel_SE": "PSPNet-ChannelAttention.py"}


def install_stub() -> None:
    """torchvision.models.{resnet, segmentation, segmentation.fcn} on top of oracle.ref_loader's transforms stub."""
    ref_loader._install_torchvision_stub()
    from insar_unet_ca_amd import deeplab, fcn

    class _RefFCN(fcn._FCN):
        def forward(self, x):
            size = x.shape[-2:]
            bb = self.backbone
            y = bb.maxpool(bb.relu(bb.bn1(bb.conv1(x))))
            for name in ("layer1", "layer2", "layer3", "layer4"):
                y = bb[name](y)
            y = self.classifier(y)
            return {"out": F.interpolate(y, size=size, mode="bilinear", align_corners=False)}

    def _bottleneck_forward(self, x):       # torchvision Bottleneck.forward (the restated class has no forward)
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)

    class Bottleneck(deeplab.Bottleneck):
        forward = _bottleneck_forward

    def fcn_resnet50(pretrained=False, progress=True, **_kw):
        if pretrained:
            raise NotImplementedError("stub: no downloaded weights")
        m = _RefFCN()
        for layer in ("layer1", "layer2", "layer3", "layer4"):          # make the blocks the stub's Bottleneck class
            for blk in m.backbone[layer]:
                blk.__class__ = Bottleneck
        return m

    tv = sys.modules["torchvision"]
    models = types.ModuleType("torchvision.models")
    seg = types.ModuleType("torchvision.models.segmentation")
    seg_fcn = types.ModuleType("torchvision.models.segmentation.fcn")
    resnet = types.ModuleType("torchvision.models.resnet")
    seg_fcn.FCNHead = fcn.FCNHead
    seg.fcn = seg_fcn
    seg.fcn_resnet50 = fcn_resnet50
    seg.fcn_resnet101 = fcn_resnet50
    resnet.Bottleneck = Bottleneck
    models.segmentation, models.resnet = seg, resnet
    tv.models = models
    sys.modules.update({"torchvision.models": models, "torchvision.models.segmentation": seg,
                        "torchvision.models.segmentation.fcn": seg_fcn, "torchvision.models.resnet": resnet})


def load_reference(script: str):
    install_stub()
    spec = importlib.util.spec_from_file_location("ref_" + script.replace("-", "_").replace(".py", ""),
                                                  os.path.join(ref_loader.REFERENCE_ROOT, script))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fingerprint(t: torch.Tensor) -> list:
    a = t.detach().double().reshape(-1)
    n = a.numel()
    idx = [0, n // 2, n - 1] if n else []
    return [float(a.sum()), float((a * a).sum())] + [float(a[i]) for i in idx]


def contract(cls) -> dict:
    torch.manual_seed(0)
    net = cls(num_classes=2, backbone="resnet50", pretrained=False)
    sd = net.state_dict()
    return {"entries": len(sd), "parameters": len(list(net.parameters())),
            "parameter_elements": int(sum(p.numel() for p in net.parameters())),
            "keys": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()],
            "dtypes": [str(v.dtype).replace("torch.", "") for v in sd.values()],
            "fingerprints": [fingerprint(v) for v in sd.values()]}


def summarise(prefix: str, a64: torch.Tensor, a32: torch.Tensor, store: dict, full: bool = True) -> None:
    a = a64.detach().double().reshape(-1).numpy()
    b = a32.detach().double().reshape(-1).numpy()
    store[f"{prefix}/norm"] = np.array(np.sqrt((a * a).sum()))
    store[f"{prefix}/sum"] = np.array(a.sum())
    store[f"{prefix}/absmax"] = np.array(np.abs(a).max() if a.size else 0.0)
    store[f"{prefix}/samples"] = a[cf.sample_indices(a.size, NSAMPLE)]
    den = np.abs(a).max()
    store[f"{prefix}/noise"] = np.array(np.abs(a - b).max() / den if den > 0 else np.abs(b).max())
    if full and a.size <= FULL_LIMIT:
        store[f"{prefix}/full"] = a64.detach().double().numpy().reshape(a64.shape).copy()


def block_module(ref, layer: str, idx: int) -> nn.Module:
    """The reference's BottleneckWithSE at `layer[idx]` of its FCN-SE, with closed-form weights and BatchNorm buffers."""
    torch.manual_seed(0)
    net = ref.FCN_SingleChannel_SE(num_classes=2)
    blk = net.model.backbone[layer][idx]
    blk.load_state_dict(cf.fill_state_dict_random(blk.state_dict(), seed=BLOCK_SEED))
    return blk


def block_run(blk, shape, training: bool, dtype) -> list:
    blk = copy.deepcopy(blk).to(dtype).train(training)
    x0 = cf.make_input_random(shape, seed=BLOCK_X_SEED).to(dtype)
    steps = []
    g = None
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        for p in blk.parameters():
            p.grad = None
        out = blk(x)
        if g is None:
            g = cf.make_input_random(tuple(out.shape), seed=BLOCK_G_SEED).to(dtype)
        out.backward(g)
        steps.append({"out": out.detach().clone(), "dx": x.grad.clone(),
                      **{f"grad/{k}": p.grad.clone() for k, p in blk.named_parameters()},
                      **{f"buf/{k}": b.clone() for k, b in blk.named_buffers() if not k.endswith("num_batches_tracked")}})
    return steps


def gen_blocks(ref) -> dict:
    store = {}
    for tag, layer, idx, shape in BLOCK_CASES:
        blk = block_module(ref, layer, idx)
        for training in (True, False):
            mode = "train" if training else "eval"
            r64, r32 = block_run(blk, shape, training, torch.float64), block_run(blk, shape, training, torch.float32)
            for s in range(2):
                for k in r64[s]:
                    if s == 0 or k.startswith("buf/"):      # (the weights do not move: step 1 repeats step 0 but for the buffers)
                        summarise(f"{tag}/{mode}/step{s}/{k}", r64[s][k], r32[s][k], store, full=False)
        store[f"{tag}/shape"] = np.array(shape)
    return store


def net_setup(ref, name: str, dtype) -> nn.Module:
    torch.manual_seed(0)
    net = getattr(ref, name)(num_classes=2)
    net.load_state_dict(cf.fill_state_dict_random(net.state_dict(), seed=NET_SEED))
    net.model.classifier[3].p = 0.0
    return net.to(dtype)


def net_inputs():
    return (cf.make_input_random(NET_SHAPE, seed=NET_X_SEED),
            cf.make_target_random((NET_SHAPE[0],) + NET_SHAPE[2:], seed=NET_T_SEED, ignore_frac=0.05))


def net_run(ref, name: str, dtype) -> dict:
    x, tgt = net_inputs()
    x = x.to(dtype)
    crit = nn.CrossEntropyLoss(ignore_index=255)
    out = {}
    net = net_setup(ref, name, dtype).train()
    logits = net(x)
    loss = crit(logits, tgt)
    loss.backward()
    out["train/logits"] = logits.detach().clone()
    out["train/loss"] = loss.detach().reshape(1)
    for k, p in net.named_parameters():
        out[f"train/gradnorm/{k}"] = p.grad.detach().norm().reshape(1)
    net_e = net_setup(ref, name, dtype).eval()
    with torch.no_grad():
        out["eval/logits"] = net_e(x).clone()
    net_a = net_setup(ref, name, dtype).train()
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


def gen_net(refs) -> dict:
    store = {}
    for name, ref in refs.items():
        r64, r32 = net_run(ref, name, torch.float64), net_run(ref, name, torch.float32)
        for k in r64:
            summarise(f"{name}/{k}", r64[k], r32[k], store)
    return store


def generate() -> dict:
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    refs = {cls_name: load_reference(script) for cls_name, script in SCRIPTS.items()}
    out = {"num_classes": 2, "seed": 0}
    for cls_name, ref in refs.items():
        out[cls_name] = contract(getattr(ref, cls_name))
    return {"contract": out, "blocks": gen_blocks(refs["FCN_SingleChannel_SE"]), "net": gen_net(refs)}


def main() -> None:
    for script in SCRIPTS.values():
        if not os.path.isfile(os.path.join(ref_loader.REFERENCE_ROOT, script)):
            raise SystemExit(f"{script} not found under {ref_loader.REFERENCE_ROOT}")
    res = generate()
    with open(OUT, "w") as f:
        json.dump(res["contract"], f, indent=0)
        f.write("\n")
    np.savez_compressed(os.path.join(GOLDEN, "g12_se_bottleneck.npz"), **res["blocks"])
    np.savez_compressed(os.path.join(GOLDEN, "g12_fcn.npz"), **res["net"])
    for name in ("g12_fcn_contract.json", "g12_se_bottleneck.npz", "g12_fcn.npz"):
        print(name, os.path.getsize(os.path.join(GOLDEN, name)), "bytes")


if __name__ == "__main__":
    main()
