"""CPU-only: the launch sequence of the three networks on the ResNet-50 trunk (DeepLabV3-CA, FCN, FCN-SE) against the
sequence recorded in tests/golden/resnet_plan_launches.json (tools/gen_golden_resnet_plans.py) before the trunk was
shared: every entry point the plan calls through the C ABI, geometry queries included, in order, forward and backward;
the backward-stage tags the plan reports to a data-parallel hook and the launch count at which each fires; the stage ends
and the parameter order of the flat gradient buffer. A head added to the trunk must leave the other networks' entries alone.

The plans run on CPU tensors over a mocked ABI (tests/helpers.mock_abi), in fp32 (252 + 492, 223 + 443 and 255 + 443 calls)
and in bf16, where ConvUnit chooses between the per-tap and the flat row-tile kernels: there the mocked geometry queries
answer so that both sides of each choice occur (row tiles for dilations up to 2 only, 256-column per-tap tiles from 512
output channels on, statistics slabs above and below the pre-fold thresholds, the stem's included)."""
import json
import os

import pytest
import torch

from insar_unet_ca_amd import deeplab, fcn, tape
from tests.helpers import mock_abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet_plan_launches.json")
NETS = {"DeepLabV3_SingleChannel_Attn": deeplab.DeepLabV3_SingleChannel_Attn, "FCN_SingleChannel": fcn.FCN_SingleChannel,
        "FCN_SingleChannel_SE": fcn.FCN_SingleChannel_SE}
SHAPE = (2, 1, 64, 64)
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
ANSWERS = {
    "insar_conv7x7s2_fwd_rows": lambda B, H: B * H // 2,
    "insar_conv7x7s2_wgrad_blocks": lambda B, h2: min(B * h2, 256),
    "insar_conv3x3_flat_rows_dil_ok": lambda x, N, d: int(d <= 2),
    "insar_igemm_tile_cols_dt": lambda M, N, code: 256 if N >= 512 else 128,
    "insar_conv3x3_flat_stat_rows": lambda x, N, flags: 2048 if N >= 256 else 16,
}
ANSWERS_BF16 = dict(ANSWERS, insar_conv7x7s2_fwd_rows=lambda B, H: 8 * B * H)


def record(monkeypatch, name: str, dtype: str) -> dict:
    """One training step of NETS[name] over the mocked ABI, and a second one (a fresh network) with a recording on_bucket hook."""
    calls = mock_abi(monkeypatch, ANSWERS_BF16 if dtype == "bfloat16" else ANSWERS)
    monkeypatch.setattr(tape, "MODE", "0")
    out = {}
    for hooked in (False, True):
        net = NETS[name](num_classes=2, compute_dtype=DTYPES[dtype]).train()
        tags = []
        if hooked:
            net._hooks["on_bucket"] = lambda plan, tag: tags.append([list(tag), len(calls)])
        del calls[:]
        y = net(torch.zeros(SHAPE))
        fwd = list(calls)
        del calls[:]
        y.sum().backward()
        if hooked:
            assert (fwd, list(calls)) == (out["forward"], out["backward"]), "the hook changed the launch sequence"
            out["on_bucket"] = tags
        else:
            out["forward"], out["backward"] = fwd, list(calls)
    plan = next(iter(net._plans.plans.values()))[0]
    out["stage_ends"] = list(plan.stage_ends)
    out["grad_param_shapes"] = [list(p.shape) for p in plan.grad_params]
    return out


@pytest.fixture(scope="module")
def golden_launches():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(NETS))
def test_launch_sequence_matches_the_recording(monkeypatch, golden_launches, name, dtype):
    got, want = record(monkeypatch, name, dtype), golden_launches[name][dtype]
    for key in ("forward", "backward"):
        first = next((i for i, (a, b) in enumerate(zip(got[key], want[key])) if a != b), min(len(got[key]), len(want[key])))
        assert got[key] == want[key], (f"{name} {dtype} {key}: {len(got[key])} calls against {len(want[key])} recorded, first difference "
                                       f"at {first}: {got[key][first:first + 3]} against {want[key][first:first + 3]}")
    assert got["on_bucket"] == want["on_bucket"]
    assert got["stage_ends"] == want["stage_ends"]
    assert got["grad_param_shapes"] == want["grad_param_shapes"]
