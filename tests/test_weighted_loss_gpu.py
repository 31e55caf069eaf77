"""GPU: the imbalance-aware losses (csrc/loss_weighted.hip behind insar_unet_ca_amd/loss.py) against float64 torch on the
CPU: F.cross_entropy(weight=, ignore_index=255, label_smoothing=) for the CE forms, the written-out focal expression under
autograd, plus the oracle's soft Dice for the fused objective. This file goes through the nn.Module layer; the per-launch
coverage of the four C entry points (every dispatch arm, the second grid trip, the workspaces, stray labels, non-finite logits
under ignored pixels, per-element gradient bounds) is tests/test_weighted_loss_kernels_gpu.py.

Gates are those of the unweighted kernels (tests/test_parity_gpu.py, test_fused_dice_ce_against_oracle): loss |d| <= 2e-6,
gradient max-rel <= 1e-4, for every case, focal included. max-rel is relative to the largest gradient of the batch and so says
nothing about confident pixels, whose gradients are tiny: test_focal_on_confident_pixels holds those per pixel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import closed_form as cf
from oracle import unet_ca_oracle as orc
from tests.helpers import max_rel

pytestmark = pytest.mark.gpu

LOSS_GATE, GRAD_GATE = 2e-6, 1e-4
SHAPES = [(3, 2, 32, 48), (2, 3, 16, 20), (2, 4, 8, 12), (2, 2, 15, 17), (2, 5, 16, 16)]
SHAPE_IDS = ["k2_vec4", "k3_vec4", "k4_vec4", "k2_odd_hw", "k5_generic"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _case(shape):
    """Logits and targets of test_fused_dice_ce_against_oracle: every class occurs, a fifth of the pixels ignored."""
    lg = cf.make_input(shape, 0.9) * 3.0
    base = cf.make_target((shape[0],) + shape[2:], ignore_every=5)
    n, yy, xx = torch.meshgrid(*(torch.arange(d) for d in base.shape), indexing="ij")
    tgt = torch.where(base == 255, base, (xx * 3 + yy * 5 + n * 7) % shape[1])
    return lg, tgt


def _weights(K, zero=False):
    w = torch.linspace(0.2, 3.0, K)
    if zero:
        w[K // 2] = 0.0
    return w


def focal_ref(logits, target, gamma, alpha=None, ignore_index=255):
    """mean over valid pixels of alpha[y] (1 - p_y)^gamma (-log p_y), in the dtype of logits."""
    logp = torch.log_softmax(logits, dim=1)
    valid = target != ignore_index
    safe = torch.where(valid, target, torch.zeros_like(target))
    lp = logp.gather(1, safe.unsqueeze(1)).squeeze(1)
    a = torch.ones_like(lp) if alpha is None else alpha.to(logits.dtype)[safe]
    per = a * (1.0 - lp.exp()).pow(gamma) * (-lp)
    return (per * valid).sum() / valid.sum()


def _ref(fn, lg, dtype):
    b = lg.clone().to(dtype).requires_grad_(True)
    r = fn(b)
    r.backward()
    return float(r.detach()), b.grad.detach()


def _ours(crit, lg, tgt, dev):
    a = lg.clone().to(dev).requires_grad_(True)
    out = crit.to(dev)(a, tgt.to(dev))
    out.backward()
    return out.detach(), a.grad.detach()


def _check(crit, fn, lg, tgt, dev, what):
    loss, grad = _ours(crit, lg, tgt, dev)
    rl, rg = _ref(fn, lg, torch.float64)
    dl, dg = abs(float(loss) - rl), max_rel(grad, rg)
    msg = f"{what}: loss |d| {dl:.3e} (gate {LOSS_GATE:.1e}), gradient max-rel {dg:.3e} (gate {GRAD_GATE:.1e})"
    print(msg)
    assert dl <= LOSS_GATE, msg
    assert dg <= GRAD_GATE, msg
    return loss, grad


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("zero", [False, True], ids=["uneven", "zero_weight"])
def test_weighted_smoothed_ce_against_torch_float64(dev, shape, eps, zero):
    import insar_unet_ca_amd as iu
    lg, tgt = _case(shape)
    w = _weights(shape[1], zero)
    crit = iu.CrossEntropyLoss(weight=w, ignore_index=255, label_smoothing=eps)
    fn = lambda b: F.cross_entropy(b, tgt, weight=w.to(b.dtype), ignore_index=255, label_smoothing=eps)
    _check(crit, fn, lg, tgt, dev, f"CE_w {shape} eps={eps}")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_smoothing_without_weights_against_torch_float64(dev, shape):
    import insar_unet_ca_amd as iu
    lg, tgt = _case(shape)
    crit = iu.CrossEntropyLoss(ignore_index=255, label_smoothing=0.1)
    _check(crit, lambda b: F.cross_entropy(b, tgt, ignore_index=255, label_smoothing=0.1), lg, tgt, dev, f"CE eps=0.1 {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0, 5.0])
@pytest.mark.parametrize("with_alpha", [False, True], ids=["no_alpha", "alpha"])
def test_focal_against_float64(dev, shape, gamma, with_alpha):
    import insar_unet_ca_amd as iu
    lg, tgt = _case(shape)
    alpha = _weights(shape[1]) if with_alpha else None
    crit = iu.FocalLoss(gamma=gamma, alpha=alpha, ignore_index=255)
    _check(crit, lambda b: focal_ref(b, tgt, gamma, alpha), lg, tgt, dev, f"focal {shape} gamma={gamma}")


def focal_ref_stable(logits, target, gamma, alpha, ignore_index=255):
    """focal_ref without cancellation, for float64 references on confident pixels: q = 1 - p_y from the log-sum-exp of the
    other classes, -log p_y = log1p(sum of the others / e^{z_y}). (1 - exp(lp) loses q below 1e-10 even in float64.)"""
    valid = target != ignore_index
    safe = torch.where(valid, target, torch.zeros_like(target))
    own = torch.zeros_like(logits, dtype=torch.bool).scatter_(1, safe.unsqueeze(1), True)
    others = torch.logsumexp(logits.masked_fill(own, float("-inf")), dim=1)
    zt = logits.gather(1, safe.unsqueeze(1)).squeeze(1)
    logq = others - torch.logsumexp(logits, dim=1)
    nll = torch.log1p(torch.exp(others - zt))
    per = alpha.to(logits.dtype)[safe] * torch.exp(gamma * logq) * nll
    return (per * valid).sum() / valid.sum(), logq.detach().exp()


CONFIDENT_Q = 1e-6
# Per-pixel relative gate on confident pixels. The gradient there is alpha [g q^(g-1) p log p - q^g] (d - p) / n: a product of
# some ten fp32 operations, two of which amplify: q^g = exp(g log q) carries g |log q| times the rounding of the logarithm
# and of the exponential's argument, and e_k = exp(z_k - mx) carries |z_k - mx| times that. With g <= 2 and |log q| <= 40 on
# these inputs: (2 * 40 * 2 + 40 + 10) * 6e-8 = 1.3e-5; the project's gradient gate, 1e-4, applied per pixel, leaves the hardware
# exp / log their extra ulp. A factor formed as 1 - p_t misses this by orders of magnitude (it is 0 or 6e-8 where q is 1e-9).
CONFIDENT_GATE = 1e-4


@pytest.mark.parametrize("scale", [4.0, 8.0])
@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("fused", [False, True], ids=["focal", "dice_focal_dice_weight_0"])
def test_focal_on_confident_pixels(dev, scale, gamma, fused):
    """alpha as a float ([1 - a, a]); logits scaled until hundreds of pixels have q = 1 - p_t below 1e-6 (down to 2e-8 at
    scale 4, 3e-16 at scale 8). There the gradient of EVERY class of EVERY such pixel is held relative to its own float64
    value: this is what requires q to be summed from the other classes and d_{t,t} - p_t to be q, not 1 - p_t."""
    import insar_unet_ca_amd as iu
    lg, tgt = _case((3, 2, 32, 48))
    lg = lg * scale
    alpha = torch.tensor([0.75, 0.25])
    if fused:
        crit = iu.DiceCELoss(ignore_index=255, weight=alpha, focal_gamma=gamma, dice_weight=0.0)
    else:
        crit = iu.FocalLoss(gamma=gamma, alpha=0.25, ignore_index=255)
    loss, grad = _ours(crit, lg, tgt, dev)
    b = lg.clone().double().requires_grad_(True)
    r, q = focal_ref_stable(b, tgt, gamma, alpha)
    r.backward()
    ref = b.grad
    dl, dg = abs(float(loss) - float(r.detach())), max_rel(grad, ref)
    sel = ((tgt != 255) & (q < CONFIDENT_Q)).unsqueeze(1).expand_as(ref) & (ref.abs() > 1e-30)
    assert int(sel.sum()) >= 300, int(sel.sum())
    rel = ((grad.cpu().double() - ref).abs() / ref.abs())[sel]
    msg = (f"focal confident scale={scale} gamma={gamma}: loss |d| {dl:.3e}, gradient max-rel {dg:.3e}, {int(sel.sum())} gradient "
           f"entries with q < {CONFIDENT_Q:g} (min q {float(q[tgt != 255].min()):.1e}): per-pixel max rel {float(rel.max()):.3e} "
           f"(gate {CONFIDENT_GATE:.0e})")
    print(msg)
    assert dl <= LOSS_GATE and dg <= GRAD_GATE, msg
    assert float(rel.max()) <= CONFIDENT_GATE, msg


FUSED = {"weights": dict(eps=0.0, gamma=None), "weights_smoothing": dict(eps=0.1, gamma=None),
         "focal_alpha": dict(eps=0.0, gamma=2.0), "focal_half": dict(eps=0.0, gamma=0.5), "zero_weight": dict(eps=0.1, gamma=None)}


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("mode", list(FUSED))
def test_fused_dice_ce_w_against_float64(dev, shape, mode):
    import insar_unet_ca_amd as iu
    lg, tgt = _case(shape)
    eps, gamma = FUSED[mode]["eps"], FUSED[mode]["gamma"]
    w = _weights(shape[1], zero=(mode == "zero_weight"))
    wce, wd = 0.3, 0.7
    crit = iu.DiceCELoss(ignore_index=255, ce_weight=wce, dice_weight=wd, weight=w, label_smoothing=eps, focal_gamma=gamma)
    if gamma is None:
        term = lambda b: F.cross_entropy(b, tgt, weight=w.to(b.dtype), ignore_index=255, label_smoothing=eps)
    else:
        term = lambda b: focal_ref(b, tgt, gamma, w)
    loss, _ = _check(crit, lambda b: wce * term(b) + wd * orc.soft_dice_loss(b, tgt), lg, tgt, dev, f"DiceCE_w {mode} {shape}")
    # the logged parts: [combined, CE (or focal) term, Dice]
    x = lg.clone().to(dev).requires_grad_(True)
    out = crit(x, tgt.to(dev))
    parts = out.grad_fn.parts.cpu()
    rt, _ = _ref(term, lg, torch.float64)
    rd, _ = _ref(lambda b: orc.soft_dice_loss(b, tgt), lg, torch.float64)
    assert float(parts[0]) == float(out.detach()) == float(loss)
    assert abs(float(parts[1]) - rt) <= LOSS_GATE and abs(float(parts[2]) - rd) <= LOSS_GATE, (parts.tolist(), rt, rd)


# ---- identities --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_identities(dev, shape):
    import insar_unet_ca_amd as iu
    lg, tgt = _case(shape)
    K = shape[1]
    base_l, base_g = _ours(iu.CrossEntropyLoss(ignore_index=255), lg, tgt, dev)
    # weight = ones, eps = 0 is the unweighted loss
    l1, g1 = _ours(iu.CrossEntropyLoss(weight=torch.ones(K), ignore_index=255), lg, tgt, dev)
    assert abs(float(l1) - float(base_l)) <= 1e-6 and float((g1 - base_g).abs().max()) <= 2e-8
    # gamma = 0 without alpha is cross entropy
    l0, g0 = _ours(iu.FocalLoss(gamma=0.0, ignore_index=255), lg, tgt, dev)
    assert abs(float(l0) - float(base_l)) <= 1e-6 and float((g0 - base_g).abs().max()) <= 2e-8
    # the fused objective is the sum of its parts
    w = _weights(K)
    wce, wd = 0.3, 0.7
    lf, gf = _ours(iu.DiceCELoss(ignore_index=255, ce_weight=wce, dice_weight=wd, weight=w), lg, tgt, dev)
    lc, gc = _ours(iu.CrossEntropyLoss(weight=w, ignore_index=255), lg, tgt, dev)
    ld, gd = _ours(iu.DiceLoss(ignore_index=255), lg, tgt, dev)
    assert abs(float(lf) - (wce * float(lc) + wd * float(ld))) <= 2e-6
    assert max_rel(gf, wce * gc + wd * gd) <= 1e-5
    # the weighted mean does not see a common factor of the weights
    ls, gs = _ours(iu.CrossEntropyLoss(weight=w * 7.5, ignore_index=255), lg, tgt, dev)
    assert abs(float(ls) - float(lc)) <= 1e-6 and max_rel(gs, gc) <= 1e-5


def test_default_arguments_are_bitwise_the_existing_entry_points(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    for shape in SHAPES:
        lg, tgt = _case(shape)
        B, K, HW = shape[0], shape[1], shape[2] * shape[3]
        a, t = lg.to(dev).contiguous(), tgt.to(dev).contiguous()
        nb = call("insar_ce_blocks", B * HW)
        dl = torch.empty_like(a)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ws = torch.empty(2 + 2 * nb, dtype=torch.float32, device=dev)
        call("insar_cross_entropy", ptr(a), ptr(t), B, K, HW, 255, ptr(dl), ptr(out), ptr(ws), _lib.stream_ptr())
        l, g = _ours(iu.CrossEntropyLoss(ignore_index=255), lg, tgt, dev)
        assert torch.equal(l, out[0]) and torch.equal(g, dl)
        dl2 = torch.empty_like(a)
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        ws2 = torch.empty(3 + 3 * K + nb * (2 + 3 * K), dtype=torch.float32, device=dev)
        call("insar_dice_ce", ptr(a), ptr(t), B, K, HW, 255, 1.0, 0.3, 0.7, ptr(dl2), ptr(out3), ptr(ws2), _lib.stream_ptr())
        l, g = _ours(iu.DiceCELoss(ignore_index=255, ce_weight=0.3, dice_weight=0.7), lg, tgt, dev)
        assert torch.equal(l, out3[0]) and torch.equal(g, dl2)


# ---- reproducibility ---------------------------------------------------------------------------------------------------
def test_twenty_repeats_give_one_bit_pattern(dev):
    import insar_unet_ca_amd as iu
    lg = cf.make_input_random((16, 2, 256, 256), seed=3) * 2.0
    tgt = cf.make_target_random((16, 256, 256), seed=5, ignore_frac=0.1)
    w = torch.tensor([0.2, 3.0])
    crits = {"ce_w": iu.CrossEntropyLoss(weight=w, ignore_index=255, label_smoothing=0.1),
             "focal": iu.FocalLoss(gamma=2.0, alpha=w, ignore_index=255),
             "dice_ce_w": iu.DiceCELoss(ignore_index=255, weight=w, label_smoothing=0.1),
             "dice_focal": iu.DiceCELoss(ignore_index=255, weight=w, focal_gamma=2.0)}
    a, t = lg.to(dev), tgt.to(dev)
    for name, crit in crits.items():
        crit = crit.to(dev)
        first = None
        for _ in range(20):
            x = a.clone().requires_grad_(True)
            out = crit(x, t)
            out.backward()
            got = (out.detach().clone(), x.grad.clone())
            if first is None:
                first = got
                assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[1]).all())
            else:
                assert torch.equal(first[0], got[0]) and torch.equal(first[1], got[1]), name


# ---- bf16 logits -------------------------------------------------------------------------------------------------------
def test_bf16_logits_give_a_bf16_gradient(dev):
    import insar_unet_ca_amd as iu
    lg, tgt = _case((3, 2, 32, 48))
    lg16 = lg.to(torch.bfloat16)
    w = _weights(2)
    for crit in (iu.CrossEntropyLoss(weight=w, ignore_index=255, label_smoothing=0.1), iu.FocalLoss(2.0, w),
                 iu.DiceCELoss(weight=w), iu.DiceCELoss(weight=w, focal_gamma=2.0)):
        l16, g16 = _ours(crit, lg16, tgt, dev)
        l32, g32 = _ours(crit, lg16.float(), tgt, dev)
        assert g16.dtype == torch.bfloat16 and g32.dtype == torch.float32
        assert torch.equal(l16, l32) and torch.equal(g16, g32.to(torch.bfloat16))


# ---- label histogram ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5, 16])
def test_label_histogram_equals_bincount(dev, K):
    import insar_unet_ca_amd as iu
    rng = np.random.default_rng(K)
    masks = []
    for shape in ((3, 64, 48), (2, 33, 17), (4, 128, 128)):
        m = rng.integers(0, K, size=shape)
        m[rng.random(shape) < 0.15] = 255
        masks.append(torch.from_numpy(m.astype(np.int64)))
    def want(ms):
        flat = torch.cat([m.flatten() for m in ms])
        return torch.bincount(flat[flat != 255], minlength=K), int((flat == 255).sum())
    got, ign = iu.label_histogram(masks[0].to(dev), K, return_ignored=True)
    assert got.dtype == torch.int64 and torch.equal(got, want(masks[:1])[0]) and ign == want(masks[:1])[1]
    got = iu.label_histogram([m.to(dev) for m in masks], K)
    assert torch.equal(got, want(masks)[0])
    got = iu.label_histogram([(None, m) for m in masks], K, device=dev)         # (image, mask) batches from a CPU loader
    assert torch.equal(got, want(masks)[0])
    got = iu.label_histogram(masks[0].to(dev).to(torch.uint8), K)
    assert torch.equal(got, want(masks[:1])[0])
    bad = masks[0].clone()
    bad[0, 0, 0] = K
    with pytest.raises(iu.InsarError, match="outside"):
        iu.label_histogram(bad.to(dev), K)


# ---- in the training loop ----------------------------------------------------------------------------------------------
def _criteria():
    import insar_unet_ca_amd as iu
    return {"dice_ce_w": lambda: iu.DiceCELoss(ignore_index=255, weight=[0.3, 1.7]),
            "focal": lambda: iu.FocalLoss(gamma=2.0, alpha=[0.3, 1.7], ignore_index=255)}


@pytest.mark.parametrize("name", ["dice_ce_w", "focal"])
def test_training_lowers_the_loss(dev, name):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.data import make_batch
    torch.manual_seed(1)
    net = iu.UNet(1, 2, True).to(dev).train()
    crit = _criteria()[name]().to(dev)
    opt = iu.Adam(net.parameters(), lr=1e-3)
    x, y = (t.to(dev) for t in make_batch(0, 2, 64, channels=1))
    losses = []
    for _ in range(8):
        opt.zero_grad(set_to_none=True)
        l = crit(net(x), y)
        l.backward()
        opt.step()
        losses.append(float(l))
    print(name, losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def _train(dev, name, graphed, steps, batches):
    import insar_unet_ca_amd as iu
    torch.manual_seed(3)
    net = iu.UNet(2, 2, True, compute_dtype=torch.float32).to(dev).train()
    crit = _criteria()[name]().to(dev)
    opt = iu.Adam(net.parameters(), lr=1e-3)
    losses = []
    if graphed:
        step = iu.GraphedTrainStep(net, crit, opt, batches[0][0], batches[0][1], warmup=2)
        for i in range(step.warmup_steps, steps):
            x, y = batches[i % len(batches)]
            losses.append(float(step(x, y)))
    else:
        for i in range(steps):
            x, y = batches[0] if i < 2 else batches[i % len(batches)]
            opt.zero_grad(set_to_none=True)
            l = crit(net(x), y)
            l.backward()
            opt.step()
            if i >= 2:
                losses.append(float(l))
    torch.cuda.synchronize()
    return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}, {k: p.grad.clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("name", ["dice_ce_w", "focal"])
def test_graph_replay_is_bitwise_the_eager_step(dev, name):
    from insar_unet_ca_amd.data import make_batch
    batches = [tuple(t.to(dev) for t in make_batch(4 * i, 4, 32, channels=2)) for i in range(3)]
    le, sde, ge = _train(dev, name, False, 7, batches)
    lg, sdg, gg = _train(dev, name, True, 7, batches)
    assert le == lg, (le, lg)
    for k in sde:
        assert torch.equal(sde[k], sdg[k]), k
    for k in ge:
        assert torch.equal(ge[k], gg[k]), k


@pytest.mark.parametrize("name", ["dice_ce_w", "focal"])
def test_taped_training_is_bitwise_the_ordinary_launch_code(dev, name, monkeypatch):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import tape
    from insar_unet_ca_amd.data import make_batch
    batches = [tuple(t.to(dev) for t in make_batch(4 * i, 4, 32, channels=2)) for i in range(3)]

    def run(mode):
        monkeypatch.setattr(tape, "MODE", mode)
        torch.manual_seed(4)
        net = iu.UNet(2, 2, True, compute_dtype=torch.float32).to(dev).train()
        crit = _criteria()[name]().to(dev)
        opt = iu.Adam(net.parameters(), lr=1e-3)
        losses = []
        for i in range(12):
            x, y = batches[i % len(batches)]
            opt.zero_grad(set_to_none=True)
            loss = crit(net(x), y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        plans = [pl for lst in net._plans.plans.values() for pl in (lst if isinstance(lst, list) else [lst])]
        reports = [pl.tape_report() for pl in plans if hasattr(pl, "tape_report")]
        return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}, reports

    off, on = run("0"), run("1")
    assert off[0] == on[0], (off[0], on[0])
    for k in off[1]:
        assert torch.equal(off[1][k], on[1][k]), k
    states = [v for rep in on[2] for v in rep.values()]
    assert states and all(s.startswith("replaying") for s in states), on[2]
