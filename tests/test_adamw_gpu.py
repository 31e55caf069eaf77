"""GPU: insar_unet_ca_amd.AdamW (csrc/optim_w.hip) against the float64 reference tests/optim_ref.py, one step at a time from
the float32 state the kernels left, within k * 2^-24 * U (k from the float32 floor: tests/adamw_cases.py); bitwise against
Adam where nothing new is switched on; reproducibility, schedule, non-finite skip, EMA swap, graph replay, checkpoint."""
import copy

import numpy as np
import pytest
import torch

from tests import adamw_cases as cases
from tests import optim_ref as ref

pytestmark = pytest.mark.gpu
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def values():
    return cases.make_values(steps=6)


def _place(arr, dev, unaligned):
    """Device copy of a float32 array; unaligned: a view that starts 4 bytes into its buffer."""
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    if not unaligned:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    buf[1:].copy_(t)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _make(dev, params, cls, cfg=None, **kw):
    """Parameters on the device (tensor cases.UNALIGNED misaligned) and an optimizer over them."""
    import insar_unet_ca_amd as iu
    ps = [torch.nn.Parameter(_place(p, dev, i == cases.UNALIGNED)) for i, p in enumerate(params)]
    if cls is iu.Adam:
        return ps, iu.Adam(ps, lr=cases.BASE_LR, betas=cases.BETAS, eps=cases.EPS)
    cfg = dict(cfg or {})
    groups = ps
    if cfg.pop("groups", False):
        groups = [{"params": ps[0::2]}, {"params": ps[1::2], "weight_decay": 0.0, "lr": 0.25 * cases.BASE_LR}]
    if cfg.pop("schedule", False):
        cfg["schedule"] = iu.LRSchedule(**cases.SCHEDULE)
    else:
        cfg.pop("schedule", None)
    gs = cfg.pop("grad_scale", 1.0)
    cfg.update(kw)
    opt = iu.AdamW(groups, lr=cases.BASE_LR, betas=cases.BETAS, eps=cases.EPS, **cfg)
    opt.grad_scale = gs
    return ps, opt


def _set_grads(ps, grads, dev):
    for i, (p, g) in enumerate(zip(ps, grads)):
        p.grad = _place(g, dev, i == cases.UNALIGNED)


def _ordered(ps, opt):
    """Per tensor, in the order of `ps`: (p, m, v, ema or None) as float32 arrays."""
    torch.cuda.synchronize()
    out = []
    for p in ps:
        st = opt.state[p]
        e = getattr(opt, "_ema", {}).get(p)
        out.append((p.detach().cpu().numpy().copy(), st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy(),
                    None if e is None else e.cpu().numpy().copy()))
    return out


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)) for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def test_defaults_are_bitwise_adam(dev, values):
    """weight_decay = 0, no clip, no schedule, no EMA: five steps give the parameters and moments of Adam with the device-side
    step count, on the float4 body, its element-wise tail and the unaligned path."""
    import insar_unet_ca_amd as iu
    params, grads = values
    pa, adam = _make(dev, params, iu.Adam)
    adam.enable_device_step()
    pw, adamw = _make(dev, params, iu.AdamW, dict(weight_decay=0.0))
    for t in range(5):
        _set_grads(pa, grads[t], dev)
        _set_grads(pw, grads[t], dev)
        adam.step()
        adamw.step()
        a, w = _ordered(pa, adam), _ordered(pw, adamw)
        for i, (x, y) in enumerate(zip(a, w)):
            for k, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
                assert np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)), (t, cases.SIZES[i], name)
    assert float(adamw.state_dict()["state"][0]["step"]) == float(adam.state_dict()["state"][0]["step"]) == 5.0


@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_each_step_against_float64(dev, values, name):
    params, grads = values
    cfg = cases.resolve(name, grads)
    ps, opt = _make(dev, params, None, {k: v for k, v in cfg.items()})
    state = [(p, np.zeros_like(p), np.zeros_like(p), p.copy() if cfg["ema_decay"] is not None else None) for p in params]
    worst = [0.0] * 4
    for t in range(1, cases.STEPS + 1):
        _set_grads(ps, grads[t - 1], dev)
        opt.step()
        got = _ordered(ps, opt)
        blk = opt._read_state()
        assert blk["t"] == t and blk["skip"] == 0
        coef = None
        if cfg["max_grad_norm"] is not None:
            norm = ref.grad_norm(grads[t - 1], cfg["grad_scale"])
            _, _, unit = ref.norm_unit(grads[t - 1], cfg["grad_scale"])
            print(f"{name} t={t} norm ratio {abs(blk['grad_norm'] - norm) / (EPS24 * unit):.3f}")
            assert abs(blk["grad_norm"] - norm) <= cases.K["norm"] * EPS24 * unit
            want = ref.clip_coef(norm, cfg["max_grad_norm"])
            if want < 1.0:                                        # relative error of the norm, plus the coefficient's own rounding
                assert abs(blk["coef"] - want) <= want * (cases.K["norm"] * EPS24 * unit / norm + EPS24)
            else:
                assert blk["coef"] == 1.0
            coef = blk["coef"]
        _, _, _, want, units = cases.reference_step(cfg, t, state, grads[t - 1], coef=coef)
        r = cases.ratios(got, want, units)
        print(f"{name} t={t} ratios p {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f} ema {r[3]:.3f}")
        worst = [max(a, b) for a, b in zip(worst, r)]
        state = got
    for k, kind in enumerate(("p", "m", "v", "ema")):
        assert worst[k] <= cases.K[kind], (name, kind, worst[k], cases.K[kind])


def test_norm_and_clip(dev, values):
    params, grads = values
    g = grads[1]
    gs = 0.25
    norm = ref.grad_norm(g, gs)
    n, S, unit = ref.norm_unit(g, gs)
    assert norm > 1.0                                            # so the bound on the norm is also within k 2^-24 sqrt(n) S

    def run(**kw):
        ps, opt = _make(dev, params, None, dict(weight_decay=0.0, grad_scale=gs), **kw)
        _set_grads(ps, g, dev)
        opt.step()
        return _ordered(ps, opt), opt

    plain, o0 = run()
    above, o1 = run(max_grad_norm=2.0 * norm)
    got = o1.last_grad_norm()
    print(f"norm ratio {abs(got - norm) / (EPS24 * unit):.3f}")
    assert abs(got - norm) <= cases.K["norm"] * EPS24 * unit <= cases.K["norm"] * EPS24 * np.sqrt(n) * S
    assert o1._read_state()["coef"] == 1.0 and _same(plain, above)
    with pytest.raises(Exception, match="last_grad_norm"):
        o0.last_grad_norm()
    # half the norm: the update is the unclipped one on gradients scaled by the reference's coefficient
    half, o2 = run(max_grad_norm=0.5 * norm)
    coef = o2._read_state()["coef"]
    want = ref.clip_coef(norm, 0.5 * norm)
    assert 0.49 < want < 0.5 and abs(coef - want) <= want * (cases.K["norm"] * EPS24 * unit / norm + EPS24)
    cfg = cases.resolve("clip", [g])
    cfg.update(grad_scale=gs, max_grad_norm=0.5 * norm)
    state = [(p, np.zeros_like(p), np.zeros_like(p), None) for p in params]
    _, _, _, ref_out, units = cases.reference_step(cfg, 1, state, g, coef=coef)
    r = cases.ratios(half, ref_out, units)
    assert all(r[k] <= cases.K[kind] for k, kind in enumerate(("p", "m", "v"))), r
    assert not _same(plain, half)


def _full_run(dev, params, grads, steps=6):
    cfg = cases.resolve("all", grads)
    ps, opt = _make(dev, params, None, cfg)
    for t in range(steps):
        _set_grads(ps, grads[t], dev)
        opt.step()
    out = _ordered(ps, opt)
    return out, np.float32(opt.last_grad_norm())


def test_reproducible(dev, values):
    params, grads = values
    first, norm0 = _full_run(dev, params, grads)
    for _ in range(19):
        again, norm = _full_run(dev, params, grads)
        assert _same(first, again) and norm.view(np.uint32) == norm0.view(np.uint32)


@pytest.mark.parametrize("kind", ["constant", "cosine", "poly"])
def test_schedule_on_the_device(dev, kind, monkeypatch):
    import insar_unet_ca_amd as iu
    base = 3e-3
    sched = iu.LRSchedule(kind, 12, warmup_steps=3, warmup_start=0.1, min_lr=1e-5, power=0.9)
    p = torch.nn.Parameter(torch.ones(5, device=dev))
    opt = iu.AdamW([p], lr=base, schedule=sched)
    p.grad = torch.ones_like(p)
    seen = []
    for t in range(1, 16):
        opt.step()
        seen.append(opt._read_state()["lr"])
    monkeypatch.setattr(opt, "_read_state", lambda: pytest.fail("get_last_lr must not read the device"))
    assert opt.get_last_lr() == [sched.lr_at(base, 14)] and opt.param_groups[0]["lr"] == base
    for t, lr in enumerate(seen, start=1):
        want = np.float32(sched.lr_at(base, t - 1))
        assert abs(np.float32(lr) - want) <= np.spacing(want), (kind, t, lr, want)
    assert seen[0] == np.float32(base * 0.1) and seen[14] == np.float32(base if kind == "constant" else 1e-5)


def test_nonfinite_step_is_skipped(dev, values):
    params, grads = values
    cfg = cases.resolve("all", grads)
    ps, opt = _make(dev, params, None, cfg, skip_nonfinite=True)
    for t in range(2):
        _set_grads(ps, grads[t], dev)
        opt.step()
    before = _ordered(ps, opt)
    blk0 = opt._read_state()
    bad = [g.copy() for g in grads[2]]
    bad[7][12345] = np.inf
    _set_grads(ps, bad, dev)
    opt.step()
    blk = opt._read_state()
    assert _same(before, _ordered(ps, opt))
    assert blk["t"] == blk0["t"] == 2 and blk["skip"] == 1 and opt.skipped_steps() == 1 and np.isinf(blk["grad_norm"])
    assert (blk["lr"], blk["bc1"], blk["bc2_sqrt"], blk["ema_alpha"]) == (blk0["lr"], blk0["bc1"], blk0["bc2_sqrt"], blk0["ema_alpha"])
    assert opt.get_last_lr()[0] == ref.lr_at(base_lr=cases.BASE_LR, t=1, **cases.SCHEDULE)
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0 and opt.state_dict()["insar_adamw"]["skipped"] == 1
    # the next finite step is the reference's step 3
    _set_grads(ps, grads[2], dev)
    opt.step()
    got = _ordered(ps, opt)
    blk = opt._read_state()
    assert blk["t"] == 3 and blk["skip"] == 0 and opt.skipped_steps() == 1
    _, _, _, want, units = cases.reference_step(cfg, 3, before, grads[2], coef=blk["coef"])
    r = cases.ratios(got, want, units)
    assert all(r[k] <= cases.K[kind] for k, kind in enumerate(("p", "m", "v", "ema"))), r
    # without the check and without clipping the norm launch is not issued (_lib's launch tape lists what was enqueued)
    from insar_unet_ca_amd import _lib
    ps2, opt2 = _make(dev, params, None, dict(weight_decay=0.0))
    _set_grads(ps2, grads[0], dev)
    _lib._TAPE = []
    try:
        opt2.step()
        names = [n for _, _, n in _lib._TAPE]
    finally:
        _lib._TAPE = None
    assert names == ["insar_optw_advance", "insar_adamw_step"]


def _unet(dev, seed=5):
    import insar_unet_ca_amd as iu
    torch.manual_seed(seed)
    return iu.UNet(1, 2, True, compute_dtype=torch.float32).to(dev).train()


def _batches(dev, n=3):
    from insar_unet_ca_amd.data import make_batch
    return [tuple(t.to(dev) for t in make_batch(2 * i, 2, 32, channels=1)) for i in range(n)]


def _recipe(net, **kw):
    import insar_unet_ca_amd as iu
    args = dict(lr=1e-3, max_grad_norm=1.0, ema_decay=0.9, schedule=iu.LRSchedule("poly", 20, warmup_steps=2, warmup_start=0.1))
    args.update(kw)
    return iu.AdamW(iu.split_decay_groups(net, 1e-2), **args)


def _eager(net, crit, opt, batches, first, n):
    out = []
    for i in range(first, first + n):
        x, y = batches[i % len(batches)]
        opt.zero_grad(set_to_none=True)
        l = crit(net(x), y)
        l.backward()
        opt.step()
        out.append(float(l.detach()))
    return out


def test_ema_weights_swap(dev):
    import insar_unet_ca_amd as iu
    net, batches = _unet(dev), _batches(dev)
    opt = iu.AdamW(net.parameters(), lr=1e-2, ema_decay=0.9)
    _eager(net, iu.CrossEntropyLoss(ignore_index=255), opt, batches, 0, 3)
    x = batches[0][0]
    net.eval()
    with torch.no_grad():
        live = net(x).clone()
        twin = iu.UNet(1, 2, True, compute_dtype=torch.float32).to(dev).eval()
        sd = opt.ema_state_dict(net)
        assert list(sd) == list(net.state_dict())
        twin.load_state_dict(sd)
        want = twin(x).clone()
        with opt.ema_weights():
            inside = net(x).clone()
        after = net(x).clone()
    assert torch.equal(inside, want) and not torch.equal(inside, live)
    assert torch.equal(after, live)


def test_graph_replay_is_bitwise_the_eager_steps(dev):
    import insar_unet_ca_amd as iu
    batches = _batches(dev)
    crit = iu.DiceCELoss(ignore_index=255)
    net_e = _unet(dev)
    opt_e = _recipe(net_e)
    # the warm-up of the graphed run uses its first batch twice
    le = _eager(net_e, crit, opt_e, [batches[0]], 0, 2) + _eager(net_e, crit, opt_e, batches, 2, 6)
    net_g = _unet(dev)
    opt_g = _recipe(net_g)
    step = iu.GraphedTrainStep(net_g, crit, opt_g, batches[0][0], batches[0][1], warmup=2)
    lg = [float(step(*batches[i % 3])) for i in range(2, 8)]
    torch.cuda.synchronize()
    assert le[2:] == lg
    for (k, a), b in zip(net_e.state_dict().items(), net_g.state_dict().values()):
        assert torch.equal(a, b), k
    for pe, pg in zip(net_e.parameters(), net_g.parameters()):
        assert torch.equal(opt_e._ema[pe], opt_g._ema[pg])
    assert opt_g.get_last_lr() == opt_e.get_last_lr() and opt_g._read_state() == opt_e._read_state()
    assert float(opt_g.state_dict()["state"][0]["step"]) == 8.0


def test_checkpoint_resumes_bitwise(dev):
    import insar_unet_ca_amd as iu
    batches = _batches(dev)
    crit = iu.CrossEntropyLoss(ignore_index=255)
    net = _unet(dev)
    opt = _recipe(net)
    _eager(net, crit, opt, batches, 0, 4)
    ck_model, ck_opt = copy.deepcopy(net.state_dict()), copy.deepcopy(opt.state_dict())
    tail = _eager(net, crit, opt, batches, 4, 4)
    net2 = _unet(dev, seed=11)
    net2.load_state_dict(ck_model)
    opt2 = _recipe(net2)
    opt2.load_state_dict(copy.deepcopy(ck_opt))
    assert opt2.get_last_lr() == [opt2.schedule.lr_at(1e-3, 3)] * 2
    tail2 = _eager(net2, crit, opt2, batches, 4, 4)
    torch.cuda.synchronize()
    assert tail == tail2
    for (k, a), b in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(a, b), k
    for pa, pb in zip(net.parameters(), net2.parameters()):
        assert torch.equal(opt._ema[pa], opt2._ema[pb])
    assert opt._read_state() == opt2._read_state() and opt2._read_state()["t"] == 8
    # torch's own AdamW takes the same dict on the CPU
    cpu = iu.UNet(1, 2, True)
    topt = torch.optim.AdamW(iu.split_decay_groups(cpu, 1e-2), lr=1e-3)
    topt.load_state_dict(copy.deepcopy(ck_opt))
    st = topt.state[next(cpu.parameters())]
    assert float(st["step"]) == 4.0 and st["exp_avg"].device.type == "cpu"


def test_train_model_takes_adamw(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(0)
    net = iu.UNet(1, 2, True).to(dev)
    opt = iu.AdamW(iu.split_decay_groups(net, 1e-2), lr=1e-3, max_grad_norm=1.0, ema_decay=0.99,
                   schedule=iu.LRSchedule("poly", 4, warmup_steps=1, warmup_start=0.1))
    train_dl = torch.utils.data.DataLoader(iu.SyntheticTiles(8, 32, channels=1), batch_size=2, shuffle=False)
    val_dl = torch.utils.data.DataLoader(iu.SyntheticTiles(2, 32, heldout=True, channels=1), batch_size=2, shuffle=False)
    hist = iu.train_model(net, train_dl, val_dl, iu.CrossEntropyLoss(ignore_index=255), opt, dev, num_epochs=1, verbose=False)
    assert len(hist) == 1 and set(hist[0]) == {"epoch", "train_loss", "train_acc", "train_miou", "train_mpa", "train_mf1",
                                               "val_loss", "val_acc", "val_miou", "val_mpa", "val_mf1"}
    assert np.isfinite(hist[0]["train_loss"]) and opt._read_state()["t"] == 4 and np.isfinite(opt.last_grad_norm())
    with opt.ema_weights():
        val = iu.validate_model(net, val_dl, iu.CrossEntropyLoss(ignore_index=255), dev, 2, verbose=False)
    assert np.isfinite(val["val_loss"])
