"""CPU-only: the SA U-Net's module surface (`insar_unet_ca_amd.spatial`) against the reference's
(Unet-SpatialAttention.py): state_dict contract, initialisation order, gradient grouping, the C descriptor's layout, and
the fixtures of tools/gen_golden_sa.py."""
import ctypes
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from insar_unet_ca_amd import _lib, engine, spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_sa", os.path.join(ROOT, "tools", "gen_golden_sa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _contract():
    with open(os.path.join(GOLDEN, "g11_unet_sa_contract.json")) as f:
        return json.load(f)


def test_state_dict_matches_the_contract():
    c = _contract()
    net = spatial.UNet(in_channels=2, num_classes=2)
    sd = net.state_dict()
    assert list(sd.keys()) == c["keys"]
    assert [list(v.shape) for v in sd.values()] == c["shapes"]
    assert len(sd) == c["entries"] == 192
    assert sum(p.numel() for p in net.parameters()) == c["parameters"] == 31043142
    assert list(sd["sa1.compress_and_map.double_conv.0.weight"].shape) == [1, 2, 3, 3]


def test_exports():
    import insar_unet_ca_amd as iu
    assert iu.UNetSpatialAttention is spatial.UNet and iu.SpatialAttention is spatial.SpatialAttention
    assert "SpatialAttention" in iu.__all__ and "UNetSpatialAttention" in iu.__all__
    sa = iu.SpatialAttention()
    assert [k for k, _ in sa.named_parameters()] == [f"compress_and_map.double_conv.{i}.{n}" for i in (0, 1, 3, 4)
                                                    for n in ("weight", "bias")]


def test_forward_refuses_cpu_tensors():
    with pytest.raises(_lib.InsarError, match="ROCm device"):
        spatial.UNet(2, 2)(torch.zeros(1, 2, 16, 16))
    with pytest.raises(_lib.InsarError, match="ROCm device"):
        spatial.SpatialAttention()(torch.zeros(1, 8, 4, 4))


@pytest.mark.parametrize("seed", [0, 1234])
def test_initialisation_matches_the_reference(seed):
    gen = _gen()
    if not gen.available():
        pytest.skip("reference tree not present")
    ref = gen.load_reference()
    torch.manual_seed(seed)
    a = ref.UNet(2, 2).state_dict()
    torch.manual_seed(seed)
    b = spatial.UNet(2, 2).state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_grad_groups_cover_every_parameter_once_with_sa_in_its_decoder_stage():
    net = spatial.UNet(2, 2)
    groups = engine.grad_groups(net)
    flat = [id(p) for g in groups for p in g]
    assert len(flat) == len(set(flat)) == len(list(net.parameters()))
    for i in range(4):
        stage = 3 - i                        # decoder stage i+1 completes as backward stage 3 - i
        ids = {id(p) for p in groups[stage]}
        sa = getattr(net, f"sa{i + 1}")
        assert all(id(p) in ids for p in sa.parameters()), i
        conv, up = getattr(net, f"conv{i + 1}"), getattr(net, f"up{i + 1}")
        order = [id(p) for p in groups[stage]]
        # completion order: conv{i+1}, then sa{i+1}, then up{i+1}
        assert order.index(id(conv.double_conv[0].weight)) < order.index(id(sa.compress_and_map.double_conv[0].weight)) \
            < order.index(id(up.weight))
    # the U-Net without SA keeps its grouping
    from insar_unet_ca_amd import UNet
    plain = engine.grad_groups(UNet(2, 2, False))
    assert [len(g) for g in plain] == [len(g) - (8 if 0 <= s < 4 else 0) for s, g in enumerate(groups)]


def test_sa_descriptor_layout_matches_the_c_compiler(tmp_path):
    header = os.path.join(ROOT, "include", "insar_hip.h")
    st = _lib.InsarSa
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){",
             'printf("size %zu\\n", sizeof(InsarSa));']
    for fname, _ in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(InsarSa, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "sa_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sa_layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if l)
    assert int(got["size"]) == ctypes.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got[fname]) == getattr(st, fname).offset, fname


def test_sa_entry_points_are_bound():
    lib = _lib.load()
    for name in ("insar_sa_compress", "insar_sa_conv", "insar_sa_gate", "insar_sa_dscale", "insar_sa_bwd_coef",
                 "insar_sa_bwd_stencil", "insar_sa_dx"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS


def test_generator_reproduces_the_committed_fixtures():
    gen = _gen()
    if not gen.available():
        pytest.skip("reference tree not present")
    out = gen.generate()
    assert out["g11_unet_sa_contract"] == _contract()
    for name in ("g11_sa_block", "g11_sa_block_full", "g11_unet_sa"):
        stored = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert sorted(stored.files) == sorted(out[name].keys())
        for k in stored.files:
            a, b = np.asarray(out[name][k], dtype=np.float64), stored[k].astype(np.float64)
            if k.endswith("/noise"):
                continue                 # a ratio of rounding errors: not a reproducible quantity at 1e-6
            den = max(float(np.abs(b).max()), 1e-30)
            assert float(np.abs(a - b).max()) <= 1e-6 * den, k
