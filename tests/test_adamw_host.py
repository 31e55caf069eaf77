"""CPU-only: the float64 reference of AdamW (tests/optim_ref.py) is pinned to torch; LRSchedule, split_decay_groups, the
constructor's refusals, the launch sequence of a step over the mocked C ABI, and the checkpoint format."""
import copy
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import AdamW, LRSchedule, _lib, optim, split_decay_groups

from tests import adamw_cases as cases
from tests import helpers
from tests import optim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED = dict(total_steps=10, warmup_steps=3, warmup_start=0.1, min_lr=1e-5, power=0.9)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("kind,decoupled", [("poly", True), ("cosine", True), ("constant", False), (None, False)])
def test_reference_is_torch_in_float64(kind, decoupled):
    """12 steps of torch.optim.AdamW (or Adam(weight_decay=), the L2 form) + clip_grad_norm_ + LambdaLR against optim_ref."""
    rng = np.random.default_rng(5)
    shapes, base, wd, max_norm, betas, eps = [(7, 5), (11,)], 3e-3, 0.05, 0.7, (0.9, 0.99), 1e-8
    ps = [torch.tensor(rng.standard_normal(s), dtype=torch.float64, requires_grad=True) for s in shapes]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(ps, lr=base, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    lam = (lambda t: ref.lr_at(kind, base, t, **SCHED) / base) if kind else (lambda t: 1.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    state = [(p.detach().numpy().copy(), np.zeros(s), np.zeros(s)) for p, s in zip(ps, shapes)]
    for t in range(1, 13):
        grads = [rng.standard_normal(s) * (3.0 if t % 2 else 0.05) for s in shapes]      # clipped on odd steps only
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(g)
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        sched.step()
        norm = ref.grad_norm(grads)
        assert abs(norm - float(total)) <= 1e-12 * norm
        coef = ref.clip_coef(norm, max_norm)
        assert (coef < 1.0) == bool(t % 2)
        lr = ref.lr_at(kind, base, t - 1, **SCHED)
        new = []
        for (p, m, v), g, tp in zip(state, grads, ps):
            (p2, m2, v2, _), _ = ref.step(p, g, m, v, None, t, lr=lr, betas=betas, eps=eps, weight_decay=wd, decoupled=decoupled, coef=coef)
            assert _rel(p2, tp.detach().numpy()) <= 1e-12, (kind, t)
            assert _rel(m2, opt.state[tp]["exp_avg"].numpy()) <= 1e-12 and _rel(v2, opt.state[tp]["exp_avg_sq"].numpy()) <= 1e-12
            new.append((p2, m2, v2))
        state = new


def test_reference_ema_is_the_averaged_model_recurrence():
    """ema += (p - ema)(1 - decay_t) is torch.optim.swa_utils' EMA update ema * d + p * (1 - d), with the warm-up decay."""
    rng = np.random.default_rng(1)
    p, e = rng.standard_normal(9), rng.standard_normal(9)
    for t, want in ((1, 2.0 / 11.0), (5, 6.0 / 15.0), (1000, 0.99)):
        d = ref.ema_decay_at(0.99, t)
        assert d == pytest.approx(want, rel=1e-15) and ref.ema_decay_at(0.99, t, warmup=False) == 0.99
        (_, _, _, e2), _ = ref.step(p, np.zeros(9), np.zeros(9), np.zeros(9), e, t, lr=0.0, ema_alpha=1.0 - d)
        fn = torch.optim.swa_utils.get_ema_multi_avg_fn(d)
        te = [torch.tensor(e)]
        fn(te, [torch.tensor(p)], None)
        assert _rel(e2, te[0].numpy()) <= 1e-12


def test_lr_schedule_points():
    base = 2e-3
    for kind in ("constant", "cosine", "poly"):
        s = LRSchedule(kind, 12, warmup_steps=3, warmup_start=0.25, min_lr=1e-5, power=0.9)
        assert s.lr_at(base, 0) == base * 0.25
        assert s.lr_at(base, 1) == base * (0.25 + 0.75 * (1 / 3))
        assert s.lr_at(base, 3) == pytest.approx(base, rel=1e-15)                    # the warm-up ends at the base rate
        for t in range(0, 20):
            assert s.lr_at(base, t) == ref.lr_at(kind, base, t, 12, 3, 0.25, 1e-5, 0.9)
        if kind == "constant":
            assert s.lr_at(base, 11) == s.lr_at(base, 12) == s.lr_at(base, 17) == base
        else:
            assert 1e-5 < s.lr_at(base, 11) < s.lr_at(base, 10) < base
            assert s.lr_at(base, 12) == 1e-5 and s.lr_at(base, 17) == 1e-5           # held at min_lr
    poly = LRSchedule("poly", 100, power=0.9)
    for t in (0, 1, 37, 99):
        assert poly.lr_at(base, t) == pytest.approx(base * (1 - t / 100) ** 0.9, rel=1e-15)
    assert poly.lr_at(base, 100) == 0.0
    cos = LRSchedule("cosine", 100, min_lr=1e-4)
    assert cos.lr_at(base, 50) == pytest.approx(1e-4 + (base - 1e-4) * 0.5, rel=1e-12)
    for bad in (dict(kind="cosine"), dict(kind="poly"), dict(kind="poly", total_steps=3, warmup_steps=3), dict(kind="step", total_steps=5),
                dict(kind="constant", warmup_steps=-1)):
        with pytest.raises(iu.InsarError):
            LRSchedule(**bad)
    assert LRSchedule("constant").lr_at(base, 10 ** 9) == base


def test_split_decay_groups():
    net = iu.UNet(1, 2, True)
    decay, exempt = split_decay_groups(net, 1e-2)
    assert decay["weight_decay"] == 1e-2 and exempt["weight_decay"] == 0.0
    ids = [id(p) for p in decay["params"] + exempt["params"]]
    assert sorted(ids) == sorted(id(p) for p in net.parameters()) and len(set(ids)) == len(ids)
    assert all(p.ndim > 1 for p in decay["params"]) and all(p.ndim <= 1 for p in exempt["params"])
    names = {id(p): n for n, p in net.named_parameters()}
    assert all(names[id(p)].endswith(("weight", "bias")) for p in exempt["params"])
    assert any("bn" in names[id(p)] or "norm" in names[id(p)].lower() or p.ndim == 1 for p in exempt["params"])


def test_constructor_refusals():
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(iu.InsarError, match="beta"):
        AdamW([{"params": [a]}, {"params": [b], "betas": (0.8, 0.999)}], lr=1e-3)
    with pytest.raises(iu.InsarError, match="max_grad_norm"):
        AdamW([a], lr=1e-3, max_grad_norm=-1.0)
    for d in (-0.1, 1.0, 1.5):
        with pytest.raises(iu.InsarError, match="ema_decay"):
            AdamW([a], lr=1e-3, ema_decay=d)
    with pytest.raises(iu.InsarError, match="total_steps"):
        AdamW([a], lr=1e-3, schedule=LRSchedule("cosine"))
    with pytest.raises(iu.InsarError, match="LRSchedule"):
        AdamW([a], lr=1e-3, schedule="poly")
    opt = AdamW([a], lr=1e-3)
    assert opt.grad_scale == 1.0 and opt.generation == 0 and opt.decoupled and opt.enable_device_step() is None
    assert not hasattr(opt, "fuse_into_backward")
    a.grad = torch.zeros(3)
    with pytest.raises(iu.InsarError, match="no CPU fallback"):
        opt.step()
    with pytest.raises(iu.InsarError):                          # the existing optimizer keeps refusing weight decay
        iu.Adam([a], weight_decay=0.1)


@pytest.fixture
def abi(monkeypatch):
    calls = helpers.mock_abi(monkeypatch)
    args = []

    def fake_call(name, *a):
        calls.append(name)
        args.append((name, a))
        return 0

    monkeypatch.setattr(optim, "call", fake_call)
    monkeypatch.setattr(optim, "_require_device", lambda p, g: None)
    return calls, args


def _params(n=3):
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(5 + i)) for i in range(n)]
    for p in ps:
        p.grad = torch.randn_like(p)
    return ps


def test_launch_sequence_and_table_reuse(abi):
    calls, args = abi
    ps = _params()
    opt = AdamW([{"params": ps[:2]}, {"params": ps[2:], "weight_decay": 0.0, "lr": 5e-4}], lr=1e-3, max_grad_norm=1.0, ema_decay=0.9)
    opt.step()
    assert calls == ["insar_gradnorm_partials", "insar_optw_advance", "insar_adamw_step"]
    table, _, nchunks, partials, cfg = next(iter(opt._tables.values()))
    assert table.shape == (3, 8) and nchunks == 3 and partials.shape == (3,)
    rows = table.tolist()
    for r, p in zip(rows, ps):
        assert r[0] == p.data_ptr() and r[1] == p.grad.data_ptr() and r[4] == opt._ema[p].data_ptr() and r[5] == p.numel()
        assert r[2] == opt.state[p]["exp_avg"].data_ptr() and r[3] == opt.state[p]["exp_avg_sq"].data_ptr()
    bits = lambda x: np.float32(x).view(np.uint32)
    assert [r[6] for r in rows] == [bits(1e-2), bits(1e-2), bits(0.0)] and [r[7] for r in rows] == [bits(1.0), bits(1.0), bits(0.5)]
    assert (cfg.lr, cfg.max_norm, cfg.ema_decay, cfg.schedule, cfg.skip_nonfinite, cfg.ema_warmup) == (1e-3, 1.0, 0.9, _lib.SCHED_NONE, 0, 1)
    first = [a for _, a in args]
    for _ in range(3):
        opt.step()
    assert calls == ["insar_gradnorm_partials", "insar_optw_advance", "insar_adamw_step"] * 4 and len(opt._tables) == 1
    strip = lambda a: tuple(x for x in a if not isinstance(x, type(ctypes.byref(cfg))))
    for i, (_, a) in enumerate(args):
        assert strip(a) == strip(first[i % 3])                   # launch arguments never change from step to step
    ps[1].grad = ps[1].grad.clone()                              # a pointer changes: the table is rebuilt, once
    opt.step(); opt.step()
    assert len(opt._tables) == 2
    # no clipping, no non-finite check: no norm launch, no workspace
    del calls[:]
    opt2 = AdamW(_params(), lr=1e-3)
    opt2.step(); opt2.step()
    assert calls == ["insar_optw_advance", "insar_adamw_step"] * 2
    assert next(iter(opt2._tables.values()))[3] is None
    adv = [a for n, a in args if n == "insar_optw_advance"][-1]
    assert adv[1] == 0 and adv[2] == 0
    del calls[:]
    opt3 = AdamW(_params(), lr=1e-3, skip_nonfinite=True)
    opt3.step()
    assert calls[0] == "insar_gradnorm_partials"


def test_state_dict_is_torchs_plus_one_top_level_entry(abi):
    ps = _params()
    sched = LRSchedule("poly", 20, warmup_steps=2)
    opt = AdamW(ps, lr=1e-3, ema_decay=0.9, schedule=sched)
    for _ in range(4):
        opt.step()
    assert opt.get_last_lr() == [sched.lr_at(1e-3, 3)] and opt.param_groups[0]["lr"] == 1e-3
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "insar_adamw"}
    assert set(sd["insar_adamw"]) == {"skipped", "ema"} and sorted(sd["insar_adamw"]["ema"]) == [0, 1, 2] and sd["insar_adamw"]["skipped"] == 0
    for i in range(3):
        assert set(sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][i]["step"]) == 4.0
    # torch's own optimizer takes it (unknown top-level keys are ignored) and continues from step 4
    twins = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    topt = torch.optim.AdamW(twins, lr=1e-3)
    topt.load_state_dict(copy.deepcopy(sd))      # (torch keeps same-device tensors of the dict by reference)
    assert float(topt.state[twins[0]]["step"]) == 4.0 and topt.state[twins[2]]["exp_avg"].shape == ps[2].shape
    for p in twins:
        p.grad = torch.zeros_like(p)
    topt.step()
    assert float(topt.state[twins[0]]["step"]) == 5.0
    # a fresh AdamW: state re-allocated (generation moves); a second load into it restores in place
    fresh = AdamW([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1e-3, ema_decay=0.9, schedule=sched)
    fresh.load_state_dict(copy.deepcopy(sd))
    assert fresh.generation == 1 and fresh._host_t == 4 and fresh.get_last_lr() == opt.get_last_lr()
    q = fresh.param_groups[0]["params"][1]
    assert torch.equal(fresh._ema[q], opt._ema[ps[1]]) and fresh._ema[q].data_ptr() != opt._ema[ps[1]].data_ptr()
    addr = (fresh._ema[q].data_ptr(), fresh.state[q]["exp_avg"].data_ptr(), fresh._dev_state.data_ptr())
    fresh.load_state_dict(copy.deepcopy(sd))
    assert fresh.generation == 1 and addr == (fresh._ema[q].data_ptr(), fresh.state[q]["exp_avg"].data_ptr(), fresh._dev_state.data_ptr())
    st = fresh._read_state()
    assert st["t"] == 4 and st["skipped"] == 0 and st["coef"] == 1.0


def test_ema_state_dict_and_swap(abi):
    net = iu.UNet(1, 2, True)
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    opt = AdamW(split_decay_groups(net, 1e-2), lr=1e-3, ema_decay=0.9)
    with pytest.raises(iu.InsarError, match="no EMA"):
        opt.ema_state_dict(net)
    opt.step()
    sd = opt.ema_state_dict(net)
    assert list(sd) == list(net.state_dict())
    p = next(net.parameters())
    live, version, addr = p.detach().clone(), p._version, p.data_ptr()
    opt._ema[p].add_(1.0)
    with opt.ema_weights():
        assert torch.equal(p, live + 1.0) and p._version > version and p.data_ptr() == addr
        inside = p._version
    assert torch.equal(p, live) and p._version > inside and p.data_ptr() == addr and torch.equal(opt._ema[p], live + 1.0)
    with pytest.raises(iu.InsarError, match="no EMA"):
        with AdamW(net.parameters(), lr=1e-3).ema_weights():
            pass


def test_state_and_config_layouts_match_the_c_compiler(tmp_path):
    structs = {"InsarOptwState": _lib.InsarOptwState, "InsarOptwConfig": _lib.InsarOptwConfig}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "insar_hip.h")}"', "int main(void){"]
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, st in structs.items():
        assert int(got[cname]) == ctypes.sizeof(st)
        for f, _ in st._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(st, f).offset, f"{cname}.{f}"
    assert ctypes.sizeof(_lib.InsarOptwState) == 48 == 4 * 12      # AdamW keeps the block as 12 int32 words
    assert _lib.ABI_VERSION == 8                                    # additive
    for name in ("insar_gradnorm_partials", "insar_optw_advance", "insar_adamw_step"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)


def test_entry_points_validate_before_launching():
    cfg = _lib.InsarOptwConfig(1e-3, 0.9, 0.999, -1.0, 0.0, 0.0, 0.9, -1.0, 3, 3, _lib.SCHED_POLY, 0, 1, 0)
    with pytest.raises(iu.InsarError, match="null"):
        _lib.call("insar_optw_advance", ctypes.byref(cfg), None, 0, None, None)
    with pytest.raises(iu.InsarError, match="total_steps"):
        _lib.call("insar_optw_advance", ctypes.byref(cfg), None, 0, 16, None)
    with pytest.raises(iu.InsarError, match="chunking"):
        _lib.call("insar_adamw_step", 16, 16, 1, 6, 0.9, 0.999, 1e-8, 1.0, 1, 16, None)
    with pytest.raises(iu.InsarError, match="null"):
        _lib.call("insar_gradnorm_partials", 16, 16, 1, 8, 1.0, None, None)


def test_gpu_tolerance_factors_are_twice_the_float32_floor():
    """k of tests/test_adamw_gpu.py: optim_ref's formulas in float32 with sequential sums against float64 on that file's cases,
    largest ratio per output, doubled (rounded up in the third decimal)."""
    floor = cases.float32_floor()
    assert set(floor) == set(cases.K)
    for name, r in floor.items():
        assert 0.25 < r < 1.5, (name, r)                           # the error units are neither slack nor short
        assert 2.0 * r <= cases.K[name] <= 2.0 * r + 1e-3, (name, r)
