"""GPU: the launch plan of the Adam family's host side (optim.Adam, optim.AdamW, parallel._hip_adam_rows) over three
parameters of numel 1, CHUNK and CHUNK + 1, with `_lib.call` wrapped by a recorder that passes every call through.

Script, per optimizer (AdamW with max_grad_norm and ema_decay set): a full step, a fast step, enable_device_step() and two
more steps, a state_dict() / load_state_dict() round trip and one step, one step after a gradient tensor was replaced (the
table is rebuilt); then one _hip_adam_rows launch on Adam's rows.

Asserted: the launch sequence (entry names in order, every scalar argument, nchunks, the pointer table and the chunk list
read back from the device, pointers normalised to role + tensor index); the addresses of exp_avg, exp_avg_sq, the EMA and
the device-side state, and `generation`, across the round trip; the parameters after the script, bit for bit.

PLAN and tests/golden/optim_launch_plan.npz were recorded from the code BEFORE the three table builders, the seven launch
sites of the plain Adam kernel and the two in-place state restores were folded (`python -m tests.test_optim_launch_plan_gpu
--record` prints the plan and writes the fixture); they are never regenerated from the code under test."""
import copy
import gc
import os
import pprint
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_launch_plan.npz")
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
STEPS = 6

# what each entry point's arguments are: T pointer table, C chunk list, S device-side state, P partials workspace,
# G the InsarOptwConfig by reference, Q the stream, K CHUNK, v a scalar kept as it is
LAYOUT = {
    "insar_adam_step": "TCvKvvvvvvvQ",
    "insar_adam_step_dev": "TCvKvvvvSvQ",
    "insar_gradnorm_partials": "TCvKvPQ",
    "insar_optw_advance": "GPvSQ",
    "insar_adamw_step": "TCvKvvvvvSQ",
}

# ---- the recording (the repeated parts named once) ----------------------------------------------------------------------
T5 = [["p0", "g0", "m0", "v0", 1], ["p1", "g1", "m1", "v1", 8192], ["p2", "g2", "m2", "v2", 8193]]
T8 = [["p0", "g0", "m0", "v0", "ema0", 1, 1008981770, 1065353216], ["p1", "g1", "m1", "v1", "ema1", 8192, 1008981770, 1065353216],
      ["p2", "g2", "m2", "v2", "ema2", 8193, 1008981770, 1065353216]]
CH = [[0, 0], [1, 0], [2, 0], [2, 1]]
CFG = {"lr": 0.001, "beta1": 0.9, "beta2": 0.999, "max_norm": 1.0, "warmup_start": 0.0, "min_lr": 0.0, "power": 1.0, "ema_decay": 0.9,
       "warmup_steps": 0, "total_steps": 0, "schedule": 0, "skip_nonfinite": 0, "ema_warmup": 1, "_pad": 0}
ADAM_DEV = ["insar_adam_step_dev", T5, CH, 4, "CHUNK", 0.001, 0.9, 0.999, 1e-08, "state", 1.0, "stream"]
ADAMW = [["insar_gradnorm_partials", T8, CH, 4, "CHUNK", 1.0, "partials", "stream"],
         ["insar_optw_advance", CFG, "partials", 4, "state", "stream"],
         ["insar_adamw_step", T8, CH, 4, "CHUNK", 0.9, 0.999, 1e-08, 1.0, 1, "state", "stream"]]
PLAN = [
    # Adam: a full step and a fast step on the host's step count (t = 1, 2)
    ["insar_adam_step", T5, CH, 4, "CHUNK", 0.001, 0.9, 0.999, 1e-08, 0.09999999999999998, 0.031622776601683805, 1.0, "stream"],
    ["insar_adam_step", T5, CH, 4, "CHUNK", 0.001, 0.9, 0.999, 1e-08, 0.18999999999999995, 0.04471017781221601, 1.0, "stream"],
    # enable_device_step(): two steps, the round trip and a step, a step on a replaced gradient tensor
    ADAM_DEV, ADAM_DEV, ADAM_DEV, ADAM_DEV,
    # _hip_adam_rows on the same rows (bias corrections of t = 7)
    ["insar_adam_step", T5, CH, 4, "CHUNK", 0.001, 0.9, 0.999, 1e-08, 0.5217030999999999, 0.08354061865356845, 1.0, "stream"],
    # AdamW: three launches per step, six steps
] + ADAMW * STEPS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _live_tensor(address: int, dtype) -> torch.Tensor:
    """The live device tensor of `dtype` that starts at `address` (the optimizers keep their tables alive in their caches)."""
    for o in gc.get_objects():
        if isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == dtype and o.data_ptr() == address:
            return o
    raise AssertionError(f"no live {dtype} device tensor at {address:#x}")


class Recorder:
    """Stands in for `call`: normalises what it is given, then passes the call through."""

    def __init__(self, real, roles, state_ptr):
        self.real, self.roles, self.state_ptr, self.plan = real, roles, state_ptr, []

    def __call__(self, name, *a):
        from insar_unet_ca_amd import _lib, optim
        roles, out = self.roles(), [name]
        for kind, x in zip(LAYOUT[name], a, strict=True):
            if kind == "T":
                out.append([[roles.get(w, w) for w in row] for row in _live_tensor(x, torch.int64).tolist()])
            elif kind == "C":
                out.append(_live_tensor(x, torch.int32).tolist())
            elif kind == "S":
                out.append("state" if x == self.state_ptr() else ("other", x))
            elif kind == "P":
                out.append("partials" if x else None)
            elif kind == "G":
                out.append({f: getattr(x._obj, f) for f, _ in x._obj._fields_})
            elif kind == "Q":
                out.append("stream" if x == _lib.stream_ptr() else ("other", x))
            elif kind == "K":
                out.append("CHUNK" if x == optim.CHUNK else x)
            else:
                out.append(x)
        self.plan.append(out)
        return self.real(name, *a)


def _tensors(dev):
    from insar_unet_ca_amd.optim import CHUNK
    gen = torch.Generator().manual_seed(11)
    sizes = (1, CHUNK, CHUNK + 1)
    init = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[torch.randn(n, generator=gen) * 0.1 for n in sizes] for _ in range(STEPS)]
    return init, grads


def _run(dev, monkeypatch_attr):
    """The script. Returns (plan, parameters as float32 arrays by name, addresses before / after each round trip)."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib, optim, parallel
    init, grads = _tensors(dev)
    plan, params, addresses = [], {}, {}
    for cls in (iu.Adam, iu.AdamW):
        name = cls.__name__
        ps = [torch.nn.Parameter(t.to(dev)) for t in init]
        for p in ps:
            p.grad = torch.zeros_like(p)
        kw = dict(max_grad_norm=1.0, ema_decay=0.9) if cls is iu.AdamW else {}
        opt = cls(ps, lr=LR, betas=BETAS, eps=EPS, **kw)

        def roles():
            out = {}
            for i, p in enumerate(ps):
                st = opt.state.get(p, {})
                named = {"p": p, "g": p.grad, "m": st.get("exp_avg"), "v": st.get("exp_avg_sq"), "ema": getattr(opt, "_ema", {}).get(p)}
                out.update({t.data_ptr(): f"{k}{i}" for k, t in named.items() if t is not None})
            return out

        def addr():
            return ([opt.state[p]["exp_avg"].data_ptr() for p in ps], [opt.state[p]["exp_avg_sq"].data_ptr() for p in ps],
                    [e.data_ptr() for e in getattr(opt, "_ema", {}).values()], opt._dev_state.data_ptr(), opt.generation)

        rec = Recorder(_lib.call, roles, lambda: _lib.ptr(opt._dev_state))
        monkeypatch_attr(_lib, "call", rec)
        monkeypatch_attr(optim, "call", rec)

        def step(k):
            for p, g in zip(ps, grads[k]):
                p.grad.copy_(g.to(dev))
            opt.step()

        step(0)
        step(1)
        opt.enable_device_step()
        step(2)
        step(3)
        sd = copy.deepcopy(opt.state_dict())
        before = addr()
        opt.load_state_dict(sd)
        addresses[name] = (before, addr())
        step(4)
        ps[1].grad = ps[1].grad.clone()
        step(5)
        if cls is iu.Adam:
            rows = [(p, p.grad, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in ps]
            parallel._hip_adam_rows(rows, LR, BETAS[0], BETAS[1], EPS, 1.0 - BETAS[0] ** 7, (1.0 - BETAS[1] ** 7) ** 0.5)
        torch.cuda.synchronize()
        plan += rec.plan
        monkeypatch_attr(_lib, "call", rec.real)
        monkeypatch_attr(optim, "call", rec.real)
        for i, p in enumerate(ps):
            params[f"{name}_{i}"] = p.detach().cpu().numpy().copy()
    return plan, params, addresses


@pytest.fixture(scope="module")
def ran(dev):
    with pytest.MonkeyPatch.context() as mp:
        return _run(dev, mp.setattr)


def test_launch_sequence(ran):
    plan = ran[0]
    assert [e[0] for e in plan] == [e[0] for e in PLAN]
    for i, (got, want) in enumerate(zip(plan, PLAN)):
        assert got == want, f"launch {i} ({want[0]})"


def test_addresses_survive_the_state_round_trip(ran):
    for name, (before, after) in ran[2].items():
        assert before == after, name
        assert before[4] == 0 and before[3] != 0 and (name == "Adam" or len(before[2]) == 3)


def test_parameters_bitwise(ran):
    want = np.load(FIXTURE, allow_pickle=False)
    assert sorted(want.files) == sorted(ran[1])
    for k, got in ran[1].items():
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want[k].view(np.uint32)), k


if __name__ == "__main__":
    # prints the plan; --record also writes the fixture (run on the code the literal is to be taken from)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    plan_, params_, addresses_ = _run(torch.device("cuda:0"), setattr)
    print("PLAN = " + pprint.pformat(plan_, width=150, compact=True))
    print("ADDRESSES_STABLE = " + repr({k: b == a for k, (b, a) in addresses_.items()}))
    if "--record" in sys.argv:
        np.savez_compressed(FIXTURE, **params_)
        print("wrote", FIXTURE)
