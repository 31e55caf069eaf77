"""GPU: insar_cross_entropy, insar_dice, insar_dice_ce and insar_confusion (csrc/loss_optim.hip) called directly, against the
float64 formulas of tests/tail_ref.py, with the workspace sized as loss.py sizes it and prefilled with NaN (as are the outputs:
every gradient element has to be written).

Bounds. The kernels use __expf / __logf and their own summation order, so their error is not derived and not taken from them
either: each check evaluates the same loss in plain float32 torch on the CPU (tail_ref on float32 tensors), and that
evaluation's deviation from float64 is the yardstick.
    loss:      |kernel - f64| <= 4 * max(yardstick, 1e-6)
    gradient:  max|kernel - f64| <= 4 * max(yardstick, floor),  floor = 2e-8 for Dice alone, 2e-8 / n_valid where CE takes part
               (its gradient is (p - onehot) / n_valid: the bound is on n_valid * gradient)
The floors are the tolerances of test_parity_gpu.py; the factor 4 covers a few ulp from each fast intrinsic plus the different
fold order. Every figure is printed before it is asserted (DESIGN.md "Testing the tail of the step" has the table).
Confusion counts are integers: equality."""
import math

import pytest
import torch

from tests import tail_ref as tr

pytestmark = pytest.mark.gpu
E_SHAPE = -1001
IGN = 255
# (B, HW): one pixel; around one block; 263168 pixels with HW % 4 == 0 (over the 1024-block cap: the per-pixel kernels take a
# second trip); 262167 pixels with odd HW (23 pixels into the second trip); every four-pixel group a whole image
BLOCK_SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (2, 131584), (3, 87389), (5, 4)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _logits(B, K, HW, seed, scale=3.0):
    return torch.randn((B, K, HW), generator=torch.Generator().manual_seed(seed)) * scale


def _targets(B, K, HW, seed, ignore_frac=0.15):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, K, (B, HW), generator=g)
    t = torch.where(torch.rand((B, HW), generator=g) < ignore_frac, torch.full_like(t, IGN), t)
    t[0, 0] = 0                                                # at least one valid pixel
    return t


def _nan(n, dev):
    return torch.full((n,), float("nan"), device=dev)


class Kernels:
    """The four entry points on one (logits, target) pair. `offset` floats of misalignment for logits and dlogits."""

    def __init__(self, dev, lg, tg, offset=0):
        from insar_unet_ca_amd import _lib
        self.lib, self.dev = _lib, dev
        self.B, self.K, self.HW = lg.shape
        n = lg.numel()
        self.lg_store = torch.zeros(n + 8, device=dev)
        self.lg = self.lg_store[offset:offset + n]
        self.lg.copy_(lg.reshape(-1).to(dev))
        self.tg = tg.contiguous().to(dev)
        self.offset, self.n = offset, n
        self.nb = _lib.call("insar_ce_blocks", self.B * self.HW)
        assert self.nb == min((self.B * self.HW + 255) // 256, 1024)

    def _dl(self):
        store = _nan(self.n + 8, self.dev)
        store[:self.offset] = 7.0
        store[self.offset + self.n:] = 7.0
        return store, store[self.offset:self.offset + self.n]

    def _done(self, store, dl):
        guard = torch.cat([store[:self.offset], store[self.offset + self.n:]])
        assert bool((guard == 7.0).all()), "wrote outside dlogits"
        return dl.view(self.B, self.K, self.HW).cpu()

    def cross_entropy(self):
        call, ptr = self.lib.call, self.lib.ptr
        store, dl = self._dl()
        ws, out = _nan(2 + 2 * self.nb, self.dev), _nan(1, self.dev)
        call("insar_cross_entropy", ptr(self.lg), ptr(self.tg), self.B, self.K, self.HW, IGN, ptr(dl), ptr(out), ptr(ws),
             self.lib.stream_ptr())
        return float(out[0]), self._done(store, dl)

    def dice(self, smooth=1.0):
        call, ptr = self.lib.call, self.lib.ptr
        store, dl = self._dl()
        ws, out = _nan(3 * self.K * (self.nb + 1), self.dev), _nan(1, self.dev)
        call("insar_dice", ptr(self.lg), ptr(self.tg), self.B, self.K, self.HW, IGN, smooth, ptr(dl), ptr(out), ptr(ws),
             self.lib.stream_ptr())
        return float(out[0]), self._done(store, dl)

    def dice_ce(self, smooth=1.0, wce=1.0, wd=1.0):
        call, ptr = self.lib.call, self.lib.ptr
        store, dl = self._dl()
        ws, out = _nan(3 + 3 * self.K + self.nb * (2 + 3 * self.K), self.dev), _nan(3, self.dev)
        call("insar_dice_ce", ptr(self.lg), ptr(self.tg), self.B, self.K, self.HW, IGN, smooth, wce, wd, ptr(dl), ptr(out), ptr(ws),
             self.lib.stream_ptr())
        return [float(v) for v in out.cpu()], self._done(store, dl)

    def confusion(self, counts=None):
        call, ptr = self.lib.call, self.lib.ptr
        if counts is None:
            counts = torch.full((3, self.K), -12345, dtype=torch.int64, device=self.dev)        # the entry point clears it
        call("insar_confusion", ptr(self.lg), ptr(self.tg), self.B, self.K, self.HW, IGN, ptr(counts), self.lib.stream_ptr())
        return counts.cpu()


def _hold(family, what, got, ref64, ref32, floor, scale=1.0):
    """scale * |got - ref64| <= 4 * max(scale * |ref32 - ref64|, floor), on scalars or tensors (max norm); prints the figures
    first."""
    if isinstance(got, torch.Tensor):
        assert bool(torch.isfinite(got).all()), (family, what)
        err, yard = scale * float((got.double() - ref64).abs().max()), scale * float((ref32.double() - ref64).abs().max())
    else:
        assert math.isfinite(got), (family, what, got)
        err, yard = abs(got - float(ref64)), abs(float(ref32) - float(ref64))
    bound = 4.0 * max(yard, floor)
    print("LOSSFIG %s | %s | kernel %.3e | yardstick %.3e | floor %.3e | ratio %.3f" % (family, what, err, yard, floor, err / bound))
    assert err <= bound, (family, what, err, yard, bound)


def check_all(dev, family, lg, tg, which=("ce", "dice", "dice_ce", "confusion"), offset=0, smooth=1.0, wce=1.0, wd=1.0):
    k = Kernels(dev, lg, tg, offset)
    l64, l32 = lg.double(), lg.float()
    n = int((tg != IGN).sum())
    if "ce" in which:
        loss, d = k.cross_entropy()
        (r, rd), (f, fd) = tr.cross_entropy(l64, tg, IGN), tr.cross_entropy(l32, tg, IGN)
        _hold(family, "ce loss", loss, r, f, 1e-6)
        _hold(family, "ce grad*n", d, rd, fd, 2e-8, scale=n)
        assert bool((d[(tg == IGN).unsqueeze(1).expand_as(d)] == 0).all())
    if "dice" in which:
        loss, d = k.dice(smooth)
        (r, rd), (f, fd) = tr.soft_dice(l64, tg, IGN, smooth), tr.soft_dice(l32, tg, IGN, smooth)
        _hold(family, "dice loss", loss, r, f, 1e-6)
        _hold(family, "dice grad", d, rd, fd, 2e-8)
        assert bool((d[(tg == IGN).unsqueeze(1).expand_as(d)] == 0).all())
    if "dice_ce" in which:
        out, d = k.dice_ce(smooth, wce, wd)
        r, f = tr.dice_ce(l64, tg, IGN, smooth, wce, wd), tr.dice_ce(l32, tg, IGN, smooth, wce, wd)
        for i, name in enumerate(("combined", "ce part", "dice part")):
            _hold(family, "dice_ce " + name, out[i], r[i], f[i], 1e-6)
        _hold(family, "dice_ce grad*n", d, r[3], f[3], 2e-8, scale=n)
        assert bool((d[(tg == IGN).unsqueeze(1).expand_as(d)] == 0).all())
    if "confusion" in which:
        assert torch.equal(k.confusion(), tr.confusion(lg, tg, k.K, IGN))
    return k


@pytest.mark.parametrize("K", [2, 3, 4, 5])
@pytest.mark.parametrize("B,HW", BLOCK_SHAPES)
def test_losses_block_structure(dev, B, HW, K):
    """K = 2, 3, 4 take the four-pixel kernels of insar_dice_ce where HW % 4 == 0 and the per-pixel ones elsewhere; K = 5
    always the per-pixel ones."""
    check_all(dev, "blocks", _logits(B, K, HW, 100 * K + B), _targets(B, K, HW, 7 * K + HW % 1000))


@pytest.mark.parametrize("B,HW", [(1, 257), (2, 131584)])
@pytest.mark.parametrize("K", [1, 16])
def test_losses_one_class_and_max_classes(dev, B, HW, K):
    check_all(dev, "K=1,16", _logits(B, K, HW, K + B), _targets(B, K, HW, K + 3))


@pytest.mark.parametrize("B,HW", [(1, 257), (3, 87389)])
def test_cross_entropy_and_confusion_at_21_classes(dev, B, HW):
    check_all(dev, "K=21", _logits(B, 21, HW, 21 + B), _targets(B, 21, HW, 5), which=("ce", "confusion"))


def test_dice_refuses_more_than_16_classes(dev):
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import ptr
    lib = _lib.load()
    lg, tg = torch.zeros(1, 17, 16, device=dev), torch.zeros(1, 16, dtype=torch.int64, device=dev)
    dl, out, ws = _nan(17 * 16, dev), _nan(3, dev), _nan(256, dev)
    s = _lib.stream_ptr()
    assert lib.insar_dice(ptr(lg), ptr(tg), 1, 17, 16, IGN, 1.0, ptr(dl), ptr(out), ptr(ws), s) == E_SHAPE
    assert "insar_dice" in lib.insar_last_error().decode()
    assert lib.insar_dice_ce(ptr(lg), ptr(tg), 1, 17, 16, IGN, 1.0, 1.0, 1.0, ptr(dl), ptr(out), ptr(ws), s) == E_SHAPE
    assert "insar_dice_ce" in lib.insar_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dl).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())


@pytest.mark.parametrize("B,HW", [(2, 1024), (2, 131584)])
def test_dice_ce_unaligned_fallback(dev, B, HW):
    """logits and dlogits one float into a larger buffer, K = 2, HW % 4 == 0: the per-pixel kernels, the aligned call's bound."""
    lg, tg = _logits(B, 2, HW, 31), _targets(B, 2, HW, 32)
    aligned = check_all(dev, "unaligned", lg, tg, which=("dice_ce",), wce=0.3, wd=0.7)
    off = check_all(dev, "unaligned", lg, tg, which=("dice_ce",), offset=1, wce=0.3, wd=0.7)
    assert aligned.lg.data_ptr() % 16 == 0 and off.lg.data_ptr() % 16 == 4


def _target_cases(B, K, HW):
    base = _targets(B, K, HW, 41, 0.15)
    out = {"nothing ignored": _targets(B, K, HW, 42, 0.0)}
    t = base.clone(); t[1] = IGN
    out["one image ignored"] = t
    t = base.clone(); t[t == 1] = 0
    out["class 1 never occurs"] = t
    return out


@pytest.mark.parametrize("HW", [1000, 1001])
@pytest.mark.parametrize("name", ["nothing ignored", "one image ignored", "class 1 never occurs", "class only under ignored"])
def test_losses_target_patterns(dev, name, HW):
    B, K = 3, 3
    lg = _logits(B, K, HW, 43)
    if name == "class only under ignored":
        # class 2 is labelled nowhere among the valid pixels and is the confident prediction exactly on the ignored ones
        tg = _targets(B, K, HW, 44, 0.0)
        hidden = tg == 2
        lg[:, 2, :] = torch.where(hidden, torch.full_like(lg[:, 2, :], 9.0), lg[:, 2, :] - 6.0)
        tg = torch.where(hidden, torch.full_like(tg, IGN), tg)
        assert int((tg == 2).sum()) == 0 and int(hidden.sum()) > 0
    else:
        tg = _target_cases(B, K, HW)[name]
    check_all(dev, "targets", lg, tg)


@pytest.mark.parametrize("K,HW", [(2, 1024), (3, 1001), (5, 1024)])
def test_everything_ignored(dev, K, HW):
    """What tail_ref gives (pinned in test_tail_ref_host.py): CE NaN, Dice 0, combined NaN, every gradient element exactly 0."""
    lg, tg = _logits(2, K, HW, 51), torch.full((2, HW), IGN)
    k = Kernels(dev, lg, tg)
    r_ce, r_di, r_dc = tr.cross_entropy(lg.double(), tg), tr.soft_dice(lg.double(), tg), tr.dice_ce(lg.double(), tg)
    assert math.isnan(float(r_ce[0])) and float(r_di[0]) == 0.0 and math.isnan(float(r_dc[0])) and float(r_dc[2]) == 0.0
    loss, d = k.cross_entropy()
    assert math.isnan(loss) and torch.equal(d, torch.zeros_like(d))
    loss, d = k.dice()
    assert loss == 0.0 and torch.equal(d, torch.zeros_like(d))
    out, d = k.dice_ce()
    assert math.isnan(out[0]) and math.isnan(out[1]) and out[2] == 0.0 and torch.equal(d, torch.zeros_like(d))
    assert torch.equal(k.confusion(), torch.zeros(3, K, dtype=torch.int64))


@pytest.mark.parametrize("base", [0.0, 3e4])
@pytest.mark.parametrize("K,HW", [(2, 1024), (3, 1001)])
def test_saturated_logits(dev, K, HW, base):
    """One class 160 above the others (every logit an integer, so nothing rounds even at 3e4): nothing is inf or NaN, and the
    CE gradient is 0 or +-1/n. One pixel in 64 is labelled against the saturated class, which keeps the loss O(1): the 1e-6
    floor is an absolute figure for losses of that size."""
    B = 2
    g = torch.Generator().manual_seed(61)
    hot = torch.randint(0, K, (B, HW), generator=g)
    lg = torch.full((B, K, HW), base)
    lg.scatter_(1, hot.unsqueeze(1), base + 160.0)
    tg = torch.where(torch.rand((B, HW), generator=g) < 1.0 / 64, (hot + 1) % K, hot)
    tg = torch.where(torch.rand((B, HW), generator=g) < 0.1, torch.full_like(tg, IGN), tg)
    k = check_all(dev, "saturated", lg, tg)
    n = int((tg != IGN).sum())
    loss, d = k.cross_entropy()
    dn = (d.double() * n).abs()
    assert float(torch.minimum(dn, (dn - 1.0).abs()).max()) <= 4 * 6e-8          # 0 or +-1/n, to the rounding of 1/n
    sat = (d.double() * n).gather(1, hot.unsqueeze(1)).squeeze(1)
    want = torch.where((tg != IGN) & (tg != hot), 1.0, 0.0).double()
    assert float((sat - want).abs().max()) <= 4 * 6e-8


def test_confusion_ties_and_repeated_calls(dev):
    """Exact ties between 2 and between 3 classes go to the lower index; a second call into the same counts buffer does not
    accumulate onto the first; K = 1."""
    B, K, HW = 2, 3, 1001
    lg = torch.randint(-1, 2, (B, K, HW), generator=torch.Generator().manual_seed(71)).float()     # values in {-1, 0, 1}: ties abound
    tg = _targets(B, K, HW, 72)
    top = lg.max(1, keepdim=True).values
    nties = (lg == top).sum(1)
    assert int((nties == 2).sum()) > 50 and int((nties == 3).sum()) > 50
    k = Kernels(dev, lg, tg)
    counts = torch.full((3, K), 99, dtype=torch.int64, device=dev)
    first = k.confusion(counts).clone()
    assert torch.equal(first, tr.confusion(lg, tg, K, IGN))
    lg2, tg2 = _logits(B, K, HW, 73), _targets(B, K, HW, 74)
    k2 = Kernels(dev, lg2, tg2)
    assert torch.equal(k2.confusion(counts), tr.confusion(lg2, tg2, K, IGN))
    assert torch.equal(k.confusion(counts), first)
    one = Kernels(dev, _logits(2, 1, 257, 75), _targets(2, 1, 257, 76))
    assert torch.equal(one.confusion(), tr.confusion(one.lg.view(2, 1, 257).cpu(), one.tg.cpu(), 1, IGN))
