"""CPU-only: the host side of the imbalance-aware losses (insar_unet_ca_amd/loss.py on csrc/loss_weighted.hip): what the
constructors accept and refuse, the `weight` buffer, class_weights against hand arithmetic, which entry point each
configuration reaches (the ABI mocked as in tests/test_host_logic.py), and the argument checks of the four new entry points,
which run before any launch and therefore without a device."""
import math
import warnings

import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _lib, loss


def test_constructors_accept_weight_and_label_smoothing():
    c = iu.CrossEntropyLoss(weight=[0.2, 1.0])
    assert c.weight.dtype == torch.float32 and c.weight.tolist() == pytest.approx([0.2, 1.0])
    assert iu.CrossEntropyLoss(label_smoothing=0.1).label_smoothing == pytest.approx(0.1)
    assert iu.CrossEntropyLoss(weight=torch.tensor([1.0, 2.0, 0.0], dtype=torch.float64)).weight.dtype == torch.float32
    d = iu.DiceCELoss(weight=[0.2, 1.0], label_smoothing=0.05)
    assert d.ce.weight.tolist() == pytest.approx([0.2, 1.0]) and d.focal_gamma is None
    assert iu.DiceCELoss(focal_gamma=2.0).focal_gamma == 2.0
    f = iu.FocalLoss()
    assert f.gamma == 2.0 and f.alpha is None and f.ignore_index == 255
    assert iu.FocalLoss(alpha=0.25).alpha.tolist() == pytest.approx([0.75, 0.25])
    assert iu.FocalLoss(alpha=[1.0, 2.0, 3.0]).alpha.shape == (3,)
    for name in ("FocalLoss", "class_weights", "label_histogram"):
        assert name in iu.__all__ and hasattr(iu, name)


def test_reduction_other_than_mean_still_raises():
    with pytest.raises(iu.InsarError):
        iu.CrossEntropyLoss(reduction="sum")
    with pytest.raises(iu.InsarError):
        iu.CrossEntropyLoss(weight=[1.0, 1.0], reduction="none")


@pytest.mark.parametrize("bad", [[-0.1, 1.0], [float("nan"), 1.0], [float("inf"), 1.0], [[1.0, 2.0]], []],
                         ids=["negative", "nan", "inf", "two_d", "empty"])
def test_bad_weights_raise(bad):
    with pytest.raises(iu.InsarError):
        iu.CrossEntropyLoss(weight=bad)
    with pytest.raises(iu.InsarError):
        iu.DiceCELoss(weight=bad)
    with pytest.raises(iu.InsarError):
        iu.FocalLoss(alpha=bad)


@pytest.mark.parametrize("ls", [-0.1, 1.0, 1.5, float("nan")])
def test_label_smoothing_outside_range_raises(ls):
    with pytest.raises(iu.InsarError):
        iu.CrossEntropyLoss(label_smoothing=ls)
    with pytest.raises(iu.InsarError):
        iu.DiceCELoss(label_smoothing=ls)


def test_focal_arguments():
    with pytest.raises(iu.InsarError):
        iu.FocalLoss(gamma=-1)
    with pytest.raises(iu.InsarError):
        iu.FocalLoss(alpha=1.5)
    with pytest.raises(iu.InsarError):
        iu.DiceCELoss(focal_gamma=-1.0)
    with pytest.raises(iu.InsarError):
        iu.DiceCELoss(focal_gamma=2.0, label_smoothing=0.1)


def test_weight_buffer_matches_torch_and_moves():
    w = torch.tensor([0.2, 1.0, 3.0])
    ours, theirs = iu.CrossEntropyLoss(weight=w, ignore_index=255), torch.nn.CrossEntropyLoss(weight=w, ignore_index=255)
    assert list(ours.state_dict().keys()) == list(theirs.state_dict().keys()) == ["weight"]
    assert torch.equal(ours.state_dict()["weight"], theirs.state_dict()["weight"])
    assert list(iu.CrossEntropyLoss().state_dict().keys()) == list(torch.nn.CrossEntropyLoss().state_dict().keys()) == []
    theirs.load_state_dict(ours.state_dict())
    assert ours.to("meta").weight.device.type == "meta"                  # .to() reaches it: it is a buffer, not an attribute
    assert "weight" in dict(iu.CrossEntropyLoss(weight=w).named_buffers())
    assert list(iu.DiceCELoss(weight=w).state_dict().keys()) == ["ce.weight"]
    assert list(iu.FocalLoss(alpha=w).state_dict().keys()) == ["alpha"]


def test_class_weights_against_hand_values():
    counts = [90, 10, 0]                                       # N = 100, K = 3, f = 0.9, 0.1, 0
    with pytest.warns(UserWarning, match="class"):
        inv = iu.class_weights(counts, "inverse")
    assert inv.dtype == torch.float32 and inv.tolist() == pytest.approx([100 / 270, 100 / 30, 0.0], rel=1e-6)
    with pytest.warns(UserWarning):
        med = iu.class_weights(torch.tensor(counts), "median")     # median of the present frequencies = 0.5
    assert med.tolist() == pytest.approx([0.5 / 0.9, 5.0, 0.0], rel=1e-6)
    with pytest.warns(UserWarning):
        enet = iu.class_weights(counts, "enet")
    assert enet.tolist() == pytest.approx([1 / math.log(1.92), 1 / math.log(1.12), 0.0], rel=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                          # no empty class: no warning
        assert iu.class_weights([25, 25, 25, 25]).tolist() == pytest.approx([1.0] * 4)
        assert iu.class_weights([60, 30, 10], "median").tolist() == pytest.approx([0.5, 1.0, 3.0], rel=1e-6)
    with pytest.raises(iu.InsarError):
        iu.class_weights([1, 2], "sqrt")
    with pytest.raises(iu.InsarError):
        iu.class_weights([0, 0])


@pytest.fixture
def mocked_loss_abi(monkeypatch):
    calls = []

    def fake_call(name, *a):
        calls.append((name, a))
        if name == "insar_ce_blocks":
            return min((a[0] + 255) // 256, 1024)
        return 0

    for m in (_lib, loss):
        monkeypatch.setattr(m, "call", fake_call, raising=False)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(loss, "_require_device", lambda x, who: None)
    return calls


def _launches(calls):
    return [(n, a) for n, a in calls if n != "insar_ce_blocks"]


def test_default_arguments_reach_the_unweighted_entry_points(mocked_loss_abi):
    lg = torch.zeros(2, 3, 8, 8)
    tg = torch.zeros(2, 8, 8, dtype=torch.int64)
    iu.CrossEntropyLoss(ignore_index=255)(lg, tg)
    (name, a), = _launches(mocked_loss_abi)
    assert name == "insar_cross_entropy" and len(a) == len(_lib._SIGNATURES[name]) == 10
    assert a[2:6] == (2, 3, 64, 255) and a[0] == lg.data_ptr() and a[1] == tg.data_ptr() and a[9] == 0
    del mocked_loss_abi[:]
    iu.DiceCELoss(ignore_index=255, smooth=1.0, ce_weight=0.3, dice_weight=0.7)(lg, tg)
    (name, a), = _launches(mocked_loss_abi)
    assert name == "insar_dice_ce" and len(a) == len(_lib._SIGNATURES[name]) == 13
    assert a[2:6] == (2, 3, 64, 255) and a[6:9] == pytest.approx((1.0, 0.3, 0.7)) and a[12] == 0


def test_weighted_forms_reach_the_w_entry_points(mocked_loss_abi):
    lg = torch.zeros(2, 3, 8, 8)
    tg = torch.zeros(2, 8, 8, dtype=torch.int64)
    crit = iu.CrossEntropyLoss(weight=[0.2, 1.0, 3.0], ignore_index=255, label_smoothing=0.1)
    crit(lg, tg)
    (name, a), = _launches(mocked_loss_abi)
    assert name == "insar_cross_entropy_w" and len(a) == len(_lib._SIGNATURES[name])
    assert a[2:6] == (2, 3, 64, 255) and a[6] == crit.weight.data_ptr() and a[7] == pytest.approx(0.1)
    del mocked_loss_abi[:]
    iu.CrossEntropyLoss(ignore_index=255, label_smoothing=0.1)(lg, tg)          # smoothing alone: ones for the weight
    (name, a), = _launches(mocked_loss_abi)
    assert name == "insar_cross_entropy_w" and a[6] != 0
    del mocked_loss_abi[:]
    foc = iu.FocalLoss(gamma=1.5, alpha=[1.0, 2.0, 3.0])
    foc(lg, tg)
    (name, a), = _launches(mocked_loss_abi)
    assert name == "insar_focal" and len(a) == len(_lib._SIGNATURES[name])
    assert a[5] == 255 and a[6] == pytest.approx(1.5) and a[7] == foc.alpha.data_ptr()
    del mocked_loss_abi[:]
    iu.FocalLoss()(lg, tg)
    assert _launches(mocked_loss_abi)[0][1][7] == 0                              # alpha=None: a null pointer, ones in the kernel
    del mocked_loss_abi[:]
    dce = iu.DiceCELoss(weight=[0.2, 1.0, 3.0], ce_weight=0.3, dice_weight=0.7)
    dce(lg, tg)
    (name, a), = _launches(mocked_loss_abi)
    assert name == "insar_dice_ce_w" and len(a) == len(_lib._SIGNATURES[name])
    assert a[6:9] == pytest.approx((1.0, 0.3, 0.7)) and a[9] == dce.ce.weight.data_ptr() and a[10] == 0.0 and a[11] < 0
    for kw, want in (({"label_smoothing": 0.1}, (0, 0.1, -1.0)), ({"focal_gamma": 2.0}, (0, 0.0, 2.0))):
        del mocked_loss_abi[:]
        iu.DiceCELoss(**kw)(lg, tg)
        (name, a), = _launches(mocked_loss_abi)
        assert name == "insar_dice_ce_w" and a[9] == want[0] and a[10:12] == pytest.approx(want[1:])


def test_wrong_length_or_device_raises_at_call_time(mocked_loss_abi):
    lg = torch.zeros(2, 3, 8, 8)
    tg = torch.zeros(2, 8, 8, dtype=torch.int64)
    with pytest.raises(iu.InsarError, match="3 classes"):
        iu.CrossEntropyLoss(weight=[0.2, 1.0])(lg, tg)
    with pytest.raises(iu.InsarError, match="3 classes"):
        iu.DiceCELoss(weight=[0.2, 1.0])(lg, tg)
    with pytest.raises(iu.InsarError, match="two classes"):
        iu.FocalLoss(alpha=0.25)(lg, tg)                        # the float form is the binary convention
    iu.FocalLoss(alpha=0.25)(torch.zeros(2, 2, 8, 8), tg)
    with pytest.raises(iu.InsarError, match=r"\.to\(device\)"):
        iu.CrossEntropyLoss(weight=[0.2, 1.0, 3.0]).to("meta")(lg, tg)
    # .double() / .half() convert buffers; the kernels read float[K], so a converted weight is refused, not misread
    for conv in (lambda m: m.double(), lambda m: m.to(torch.bfloat16)):
        with pytest.raises(iu.InsarError, match="float32"):
            conv(iu.CrossEntropyLoss(weight=[0.2, 1.0, 3.0]))(lg, tg)
        with pytest.raises(iu.InsarError, match="float32"):
            conv(iu.DiceCELoss(weight=[0.2, 1.0, 3.0]))(lg, tg)
        with pytest.raises(iu.InsarError, match="float32"):
            conv(iu.FocalLoss(alpha=[0.2, 1.0, 3.0]))(lg, tg)
    assert not [n for n, _ in _launches(mocked_loss_abi) if n != "insar_focal"]
    del mocked_loss_abi[:]
    crit = iu.CrossEntropyLoss(label_smoothing=0.1)
    crit(lg, tg), crit(lg, tg)
    (_, a), (_, b) = _launches(mocked_loss_abi)
    assert a[6] == b[6] != 0                                                 # the unit weight: one tensor, the same pointer
    assert list(crit.state_dict().keys()) == []                             # ... and no part of the state


def test_weighted_losses_have_no_cpu_fallback():
    lg, tg = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    for crit in (iu.CrossEntropyLoss(weight=[1.0, 2.0]), iu.CrossEntropyLoss(label_smoothing=0.1), iu.FocalLoss(),
                 iu.DiceCELoss(weight=[1.0, 2.0]), iu.DiceCELoss(focal_gamma=2.0)):
        with pytest.raises(iu.InsarError, match="no CPU fallback"):
            crit(lg, tg)
    with pytest.raises(iu.InsarError, match="no CPU fallback"):
        iu.label_histogram(tg, 2)


def test_backward_accepts_a_gradient_that_is_not_a_device_scalar():
    """loss.backward(gradient=<CPU tensor>) scales the stored gradient with torch arithmetic instead of raising."""
    dl = torch.arange(6, dtype=torch.float32).reshape(1, 2, 3)
    out = loss._scale_by(dl, torch.tensor(2.0), torch.float32)
    assert torch.equal(out, dl * 2)
    assert loss._scale_by(dl, torch.tensor(0.5, dtype=torch.float64), torch.bfloat16).dtype == torch.bfloat16


def test_new_entry_points_validate_arguments_without_a_gpu():
    """Null pointers and K > 16 are refused before any launch (the style of test_argument_validation_without_a_gpu)."""
    call = _lib.call
    p = 64                                                      # never dereferenced: every call below fails its checks first
    with pytest.raises(_lib.InsarError, match="null"):
        call("insar_cross_entropy_w", None, p, 1, 2, 16, 255, p, 0.0, p, p, p, None)
    with pytest.raises(_lib.InsarError, match="null"):
        call("insar_cross_entropy_w", p, p, 1, 2, 16, 255, None, 0.0, p, p, p, None)       # the weight vector is required here
    with pytest.raises(_lib.InsarError, match="num_classes=17"):
        call("insar_cross_entropy_w", p, p, 1, 17, 16, 255, p, 0.0, p, p, p, None)
    with pytest.raises(_lib.InsarError, match="label_smoothing"):
        call("insar_cross_entropy_w", p, p, 1, 2, 16, 255, p, 1.0, p, p, p, None)
    with pytest.raises(_lib.InsarError, match="null"):
        call("insar_focal", p, None, 1, 2, 16, 255, 2.0, None, p, p, p, None)
    with pytest.raises(_lib.InsarError, match="num_classes=17"):
        call("insar_focal", p, p, 1, 17, 16, 255, 2.0, None, p, p, p, None)
    with pytest.raises(_lib.InsarError, match="gamma"):
        call("insar_focal", p, p, 1, 2, 16, 255, -1.0, None, p, p, p, None)
    with pytest.raises(_lib.InsarError, match="null"):
        call("insar_dice_ce_w", p, p, 1, 2, 16, 255, 1.0, 1.0, 1.0, p, 0.0, -1.0, None, p, p, None)
    with pytest.raises(_lib.InsarError, match="num_classes=17"):
        call("insar_dice_ce_w", p, p, 1, 17, 16, 255, 1.0, 1.0, 1.0, p, 0.0, -1.0, p, p, p, None)
    with pytest.raises(_lib.InsarError, match="do not combine"):
        call("insar_dice_ce_w", p, p, 1, 2, 16, 255, 1.0, 1.0, 1.0, p, 0.1, 2.0, p, p, p, None)
    with pytest.raises(_lib.InsarError, match="bad shape"):
        call("insar_dice_ce_w", p, p, 0, 2, 16, 255, 1.0, 1.0, 1.0, p, 0.0, -1.0, p, p, p, None)
    with pytest.raises(_lib.InsarError, match="null"):
        call("insar_label_hist", p, 16, 2, 255, None, p, None)
    with pytest.raises(_lib.InsarError, match="num_classes=17"):
        call("insar_label_hist", p, 16, 17, 255, p, p, None)
    assert _lib.ABI_VERSION == 8
