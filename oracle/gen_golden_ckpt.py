"""TEST INFRASTRUCTURE ONLY — G10: the checkpoint contract of the reference's UNet (Unet-ChannalAttention.py:100-163),
recorded from its own class: the state_dict keys in order, their shapes and dtypes, and the per-module `_metadata`
versions that `torch.save(model.state_dict())` writes (:382-387). tests/test_data_io.py checks `.pth` interchange in
both directions against it. Re-run with:  python -m oracle.gen_golden_ckpt"""
from __future__ import annotations

import json
import os

from .gen_golden import OUT
from .ref_loader import load_reference_unet_ca

# (fixture key, UNet arguments): the reference's own default model (in_channels=1, :464) and the Unet.py equivalent
CONFIGS = (("unet_ca_in1_se", dict(in_channels=1, num_classes=2, use_se=True)),
           ("unet_in2_nose", dict(in_channels=2, num_classes=2, use_se=False)))


def contract(sd) -> dict:
    return {"keys": list(sd.keys()),
            "shapes": [list(v.shape) for v in sd.values()],
            "dtypes": [str(v.dtype).replace("torch.", "") for v in sd.values()],
            "metadata": {k: dict(v) for k, v in getattr(sd, "_metadata", {}).items()}}


def main() -> None:
    ref = load_reference_unet_ca()
    g10 = {name: contract(ref.UNet(**kw).state_dict()) for name, kw in CONFIGS}
    g10["__source__"] = "state_dict() of the reference's UNet class (Unet-ChannalAttention.py), oracle/gen_golden_ckpt.py"
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "g10_checkpoint_contract.json"), "w") as f:
        json.dump(g10, f, indent=1)
    print("wrote g10_checkpoint_contract.json:", {k: len(v["keys"]) for k, v in g10.items() if isinstance(v, dict)})


if __name__ == "__main__":
    main()
