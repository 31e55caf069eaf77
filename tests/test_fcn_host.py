"""CPU-only: the FCN drop-ins (fcn.FCN_SingleChannel, fcn.FCN_SingleChannel_SE) against the reference constructors'
contract (tests/golden/g12_fcn_contract.json, tools/gen_golden_fcn.py): state_dict keys / shapes / dtypes / order, the
seed-0 initialisation (RNG order), checkpoint round trips, refused options, input checks and the gradient layout."""
import json
import os
from collections import OrderedDict

import pytest
import torch

from insar_unet_ca_amd import _lib
from insar_unet_ca_amd.fcn import FCN_SingleChannel, FCN_SingleChannel_SE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_fcn_contract.json")
CLASSES = {"FCN_SingleChannel": FCN_SingleChannel, "FCN_SingleChannel_SE": FCN_SingleChannel_SE}


@pytest.fixture(scope="module")
def contract():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CLASSES))
def test_state_dict_contract(contract, name):
    c = contract[name]
    net = CLASSES[name](num_classes=2)
    sd = net.state_dict()
    assert list(sd.keys()) == c["keys"]
    assert [list(v.shape) for v in sd.values()] == c["shapes"]
    assert [str(v.dtype).replace("torch.", "") for v in sd.values()] == c["dtypes"]
    assert len(sd) == c["entries"] and len(list(net.parameters())) == c["parameters"]
    assert sum(p.numel() for p in net.parameters()) == c["parameter_elements"]
    # no aliases: every entry owns its storage
    ptrs = [v.data_ptr() for v in sd.values() if v.numel()]
    assert len(set(ptrs)) == len(ptrs)


def test_entry_counts():
    assert len(FCN_SingleChannel_SE().state_dict()) == 358 and len(list(FCN_SingleChannel_SE().parameters())) == 196
    assert len(FCN_SingleChannel().state_dict()) == 326 and len(list(FCN_SingleChannel().parameters())) == 164


@pytest.mark.parametrize("name", list(CLASSES))
def test_seed0_initialisation_matches_the_reference(contract, name):
    """Same seed, same initial weights as the reference constructor: the RNG is consumed in the reference's order
    (PSPNet.py replaces the head before the stem, PSPNet-ChannelAttention.py the stem before the head, then the SEBlocks)."""
    torch.manual_seed(0)
    sd = CLASSES[name](num_classes=2).state_dict()
    for (k, v), fp in zip(sd.items(), contract[name]["fingerprints"]):
        a = v.detach().double().reshape(-1)
        got = [float(a.sum()), float((a * a).sum())] + ([float(a[0]), float(a[a.numel() // 2]), float(a[-1])] if a.numel() else [])
        assert got == pytest.approx(fp, rel=1e-9, abs=1e-9), k


@pytest.mark.parametrize("name", list(CLASSES))
def test_strict_round_trip_and_aux_keys_dropped(contract, name):
    src = CLASSES[name](num_classes=2)
    g = torch.Generator().manual_seed(4)
    ref_sd = OrderedDict()
    for k, shape, dt in zip(contract[name]["keys"], contract[name]["shapes"], contract[name]["dtypes"]):
        ref_sd[k] = (torch.randn(shape, generator=g) if dt == "float32" else torch.tensor(7, dtype=torch.int64))
    dst = CLASSES[name](num_classes=2)
    dst.load_state_dict(ref_sd, strict=True)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, ref_sd[k]), k
    # a reference model built with pretrained=True carries an aux classifier the forward never uses
    aux = OrderedDict(ref_sd)
    aux["model.aux_classifier.0.weight"] = torch.zeros(256, 1024, 3, 3)
    aux["model.aux_classifier.4.bias"] = torch.zeros(21)
    dst.load_state_dict(aux, strict=True)
    with pytest.raises(RuntimeError):
        bad = OrderedDict(ref_sd)
        bad.pop("model.classifier.4.bias")
        dst.load_state_dict(bad, strict=True)
    del src


def test_refused_options():
    for cls in CLASSES.values():
        with pytest.raises(_lib.InsarError, match="pretrained"):
            cls(pretrained=True)
        with pytest.raises(ValueError, match="resnet101"):
            cls(backbone="resnet101")
        with pytest.raises(ValueError, match="Unsupported backbone"):
            cls(backbone="vgg16")


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (2, 64, 64), (1, 2, 1, 64, 64)])
def test_bad_input_shape_raises_value_error(shape):
    for name, cls in CLASSES.items():
        with pytest.raises(ValueError, match=f"{name} expected input shape"):
            cls()(torch.zeros(shape))


def test_load_backbone_state_dict_mean_reduces_an_imagenet_stem():
    net = FCN_SingleChannel_SE()
    bb = net.model.backbone
    sd = OrderedDict((k, torch.randn_like(v) if v.is_floating_point() else v) for k, v in bb.state_dict().items()
                     if ".se_block." not in k)
    sd["conv1.weight"] = torch.randn(64, 3, 7, 7)
    sd["fc.weight"], sd["fc.bias"] = torch.zeros(1000, 2048), torch.zeros(1000)
    net.load_backbone_state_dict(sd)
    assert torch.equal(bb.conv1.weight, sd["conv1.weight"].mean(dim=1, keepdim=True))
    assert torch.equal(bb["layer4"][2].conv3.weight, sd["layer4.2.conv3.weight"])


def test_sync_bn_refused():
    import torch.distributed as dist
    from insar_unet_ca_amd.parallel import DataParallel
    import socket
    created = not dist.is_initialized()
    if created:
        with socket.socket() as s:                      # a free port for this process's one-rank group
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        for cls in CLASSES.values():
            with pytest.raises(_lib.InsarError, match="sync_bn=True"):
                DataParallel(cls(), sync_bn=True)
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize("name", list(CLASSES))
def test_grad_groups_cover_every_parameter_once(name):
    """The backward stages (FCNPlan's flat gradient buffer, the DP buckets, the sharded parameter buffer) follow completion
    order: the head, then layer4 ... layer1 with the stem; every parameter once; each se_block's two weights in its block's
    stage."""
    net = CLASSES[name]()
    bb, head = net.model.backbone, net.model.classifier
    groups = net.grad_groups()
    assert len(groups) == 5
    flat = [p for g in groups for p in g]
    assert len(flat) == len({id(p) for p in flat}) == len(list(net.parameters()))
    assert [id(p) for p in groups[0]] == [id(p) for p in (head[4].weight, head[4].bias, head[0].weight, head[1].weight, head[1].bias)]
    assert {id(bb.conv1.weight), id(bb.bn1.weight), id(bb.bn1.bias)} <= {id(p) for p in groups[4]}
    for li in (1, 2, 3, 4):
        stage = {id(p) for p in groups[5 - li]}
        for blk in bb[f"layer{li}"]:
            assert {id(p) for p in blk.parameters()} <= stage
    if name == "FCN_SingleChannel_SE":
        assert sum(1 for p in flat if p.dim() == 4 and p.shape[2:] == (1, 1) and p.shape[0] * 16 == p.shape[1]) == 16


def test_se_res_apply_argument_checks():
    """insar_se_res_apply validates before touching the device: null pointers, mismatched operands, unsupported C."""
    import ctypes
    act = lambda c, dt=_lib.BF16, h=8, p=16: _lib.InsarAct(p, 2, h, 8, c, 0, c, dt, 0)
    y, res, dst = act(256), act(256), act(256)
    buf = 16
    call = lambda *a: _lib.call("insar_se_res_apply", *a)
    with pytest.raises(_lib.InsarError, match="null"):
        call(ctypes.byref(y), buf, buf, None, ctypes.byref(res), ctypes.byref(dst), None)
    with pytest.raises(_lib.InsarError, match="differ"):
        call(ctypes.byref(y), buf, buf, buf, ctypes.byref(act(256, h=4)), ctypes.byref(dst), None)
    with pytest.raises(_lib.InsarError, match="differ"):
        call(ctypes.byref(y), buf, buf, buf, ctypes.byref(res), ctypes.byref(act(256, _lib.F32)), None)
    with pytest.raises(_lib.InsarError, match="C=24"):          # 3 bf16 chunks: neither divides nor is a multiple of 256
        call(ctypes.byref(act(24)), buf, buf, buf, ctypes.byref(act(24)), ctypes.byref(act(24)), None)
    with pytest.raises(_lib.InsarError, match="null"):
        call(ctypes.byref(act(256, p=0)), buf, buf, buf, ctypes.byref(res), ctypes.byref(dst), None)
