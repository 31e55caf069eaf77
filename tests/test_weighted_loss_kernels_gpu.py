"""GPU: insar_cross_entropy_w, insar_focal, insar_dice_ce_w and insar_label_hist (csrc/loss_weighted.hip) called directly,
one launch sequence at a time, against the float64 formulas of tests/weighted_loss_ref.py. tests/test_weighted_loss_gpu.py goes
through the nn.Module layer; this file is to the weighted family what tests/test_loss_kernels_gpu.py is to the unweighted one
and takes its helpers, shapes and bound rule from there.

Every loss launch: the workspace is sized exactly as loss.py sizes it (2 + 2 nb floats; 4 + 3K + nb (3 + 3K) floats; (K+1) nb
int64) and sits, like dlogits, between guard words of 7.0 that must survive; ws, loss_out and dlogits are prefilled with NaN
(every partial the folds read and every gradient element has to be written: a word left out makes the loss NaN or is found
by the finiteness check, and no word of ws may still be NaN afterwards); the launch runs twice and the two results are
bitwise equal; every gradient element is finite and exactly 0 where the reference says the pixel is not valid.

Bounds: the rule of test_loss_kernels_gpu.py, no new number. The same formulas in plain float32 torch on the CPU give the
yardstick (their deviation from float64).
    loss:      |kernel - f64| <= 4 * max(yardstick, 1e-6)
    gradient:  max|kernel - f64| * scale <= 4 * max(yardstick * scale, 2e-8), no element excluded
scale = normaliser / largest class weight: W / max w for the CE forms, n_valid / max alpha for focal (n_valid for alpha null),
which makes the scaled gradient O(1) as n * gradient is in the unweighted file; 1 for Dice alone (ce_weight = 0).
What insar_dice_ce_w leaves in ws[0 .. 4 + 3K): n_valid and the T totals are sums of ones below 2^24, so equality; the
normaliser, its reciprocal, the numerator and the I, P totals are means of O(1) terms once divided by the normaliser (by
n_valid for I, P), which is what a loss is, so they are held by the loss rule (floor 1e-6) after that division.
On confident pixels (q = 1 - p_t < 1e-6) every gradient entry is held relative to its own float64 value by CONFIDENT_GATE of
tests/test_weighted_loss_gpu.py (derived there). Counts are integers: equality.
Saturated logits with label smoothing make a loss of O(10) (every wrong class costs 160); the 1e-6 floor is an absolute figure
for losses of O(1), so there the loss is only required to be finite and the gradient is held.

Paths (DESIGN.md "Imbalance-aware losses") and the cases that reach them:
    LW_MAIN arm lw_main_kernel<2, false> / <3, false> / <4, false>     test_block_structure K = 2, 3, 4 (CE_w), every shape
    LW_MAIN arm lw_main_kernel<2, true> / <3, true> / <4, true>        test_block_structure K = 2, 3, 4 (focal)
    LW_MAIN arm lw_main_kernel<16, false> / <16, true>                 test_block_structure K = 5; test_one_six_sixteen_classes
    second grid trip of lw_norm / lw_main / partial / grad kernels     (2, 131584) and (3, 87389) of the two tests above
    LW_V4 arms lw_dicece_partial_v4 / grad_v4 <2, false> <2, true>     test_block_structure K = 2 at HW % 4 == 0: (1, 256),
               <3, false> <3, true> <4, false> <4, true>               (2, 131584), (5, 4); K = 3, K = 4 likewise
    lw_dicece_partial_kernel / lw_dicece_grad_kernel, focal 0 and 1    test_block_structure at odd HW and at K = 5;
                                                                       test_one_six_sixteen_classes
    the unaligned fallback (K 2..4, HW % 4 == 0, pointer off 16 B)     test_dice_ce_w_unaligned_fallback
    lw_dicece_final_kernel, register branch (stride <= 15)             every insar_dice_ce_w case at K <= 4
    lw_dicece_final_kernel, looped branch (stride 18, 21, 51)          K = 5, 6, 16 of the tests above
    lw_valid on stray labels                                           test_stray_labels_count_as_ignored
    branchless lw_v4_stats / lw_v4_grad under invalid pixels           test_non_finite_logits_under_invalid_pixels (HW 1024)
    lw_hist_kernel / lw_hist_final_kernel                              test_label_hist
    every INSAR_FAIL of the four wrappers                              test_refusals_launch_nothing

Kernel changes this file forced, both in the focal factor and both found by the one-pixel cases, where a misclassified pixel
is the whole batch and the float32 yardstick is a single draw, so that the bound is the floor's 4 * 2e-8 = 8e-8:
  test_block_structure[1-1-4], p_t = 0.001, g = 5 with alpha: kernel 1.2e-6 on a scaled gradient element of 0.34. q^g was
    __expf(g * __logf(q)), g multiplies the absolute error of log q, and near q = 1 __logf is good to about 2^-21 absolute only.
    lw_powg (now the loss's) takes log q from logf(q), above q = 1/2 from log1pf(-p_t).
  test_block_structure[1-1-2], p = (0.0062, 0.9938) labelled 0, g = 2 without alpha: the two gradient elements are -+1.044, the
    kernel was off by 1.03e-7 (1.7 half-ulps of that value: the fp32 roundings of q^g, of lead - q^g and of the product with
    q), the yardstick by 1.6e-8, ratio 1.29. lw_pixel_grad now forms the focal coefficient and its products in double from the
    fp32 exponentials and rounds each element once: 1.6e-8 there, ratio 0.20.
The default-argument path does not run these kernels; the launch count is unchanged.

Measured on an MI355X, largest kernel / bound per output over all cases (the table is in DESIGN.md "Testing the tail of the
step"): CE_w loss 0.18, gradient 0.72; focal loss 0.20, gradient 0.99 (the saturated cases, where alpha[y] * (1 / n) passes
through two roundings and the yardstick's division through one; 0.26 elsewhere); Dice+CE_w combined / term / Dice 0.15 / 0.16 /
0.02, gradient 0.55, Dice alone 0.08; Dice+focal combined / term / Dice 0.13 / 0.17 / 0.02, gradient 0.47; ws normaliser /
reciprocal / numerator 0.03 / 0.03 / 0.19, I and P totals 0.01; confident pixels: 5.6e-6 of the entry's own value (gate 1e-4),
loss 0.07, gradient 0.03.
Wall time of this file on the MI355X: 5 s for the 93 cases, the slowest (K = 16 at 263168 pixels) 1.3 s."""
import math

import pytest
import torch

from tests import weighted_loss_ref as wr
from tests.test_loss_kernels_gpu import BLOCK_SHAPES, IGN, Kernels, _hold, _logits, _targets
from tests.test_weighted_loss_gpu import CONFIDENT_GATE, CONFIDENT_Q

pytestmark = pytest.mark.gpu
E_SHAPE, E_ARG = -1001, -1005
GUARD = 7.0
STRAY = [-1, None, 254, -2 ** 63]          # None stands for K
LARGE = 100000                             # pixels: above this a case runs one configuration per entry point


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- the cases (tests/test_weighted_loss_ref_host.py plants its errors on the small ones) ------------------------------------
def class_weights(K, zero=False):
    """Uneven weights 0.2 .. 3.0 (one of them 0 on request; never class 0, which _targets always labels)."""
    w = torch.linspace(0.2, 3.0, K)
    if zero and K > 1:
        w[K // 2] = 0.0
    return w


CE_GRID = [(eps, zero) for eps in (0.0, 0.1) for zero in (False, True)]
FOCAL_GRID = [(gamma, alpha) for gamma in (0.0, 0.5, 2.0, 5.0) for alpha in (False, True)]
# insar_dice_ce_w: (weights: None / "w" / "zero", label smoothing, focal gamma or None)
FUSED_MODES = {"weights": ("w", 0.0, None), "weights_eps": ("zero", 0.1, None), "focal2_alpha": ("w", 0.0, 2.0),
               "focal0": (None, 0.0, 0.0), "null": (None, 0.1, None)}
MIXES = [(0.3, 0.7), (1.0, 0.0), (0.0, 1.0)]
SMALL_SHAPES = [s for s in BLOCK_SHAPES if s[0] * s[1] < LARGE]


def block_case(B, K, HW):
    """The logits and targets of test_block_structure."""
    return _logits(B, K, HW, 100 * K + B), _targets(B, K, HW, 7 * K + HW % 1000)


def _wvec(kind, K):
    return None if kind is None else class_weights(K, kind == "zero")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


class WKernels(Kernels):
    """The weighted entry points on the buffers of Kernels. Each call launches twice into fresh NaN-prefilled buffers, checks
    the guards and the bitwise repeat, and returns CPU tensors (loss_out, dlogits [B][K][HW], ws)."""

    def _vec(self, v):
        return None if v is None else v.to(torch.float32).contiguous().to(self.dev)

    def _ws(self, n):
        store = torch.full((n + 12,), float("nan"), device=self.dev)
        store[:4] = GUARD
        store[4 + n:] = GUARD
        return store, store[4:4 + n]

    def _twice(self, name, nws, nout, args, expect_written=True):
        runs = []
        for _ in range(2):
            store, dl = self._dl()
            ws_store, ws = self._ws(nws)
            out = torch.full((nout,), float("nan"), device=self.dev)
            self.lib.call(name, *args(dl, out, ws))
            d = self._done(store, dl)
            assert bool((torch.cat([ws_store[:4], ws_store[4 + nws:]]) == GUARD).all()), name + ": wrote outside ws"
            runs.append((out.cpu(), d, ws.cpu()))
        assert _same(runs[0], runs[1]), name + ": two launches differ"
        if expect_written:
            assert not bool(torch.isnan(runs[0][2]).any()), name + ": a word of ws was never written"
        return runs[0]

    def ce_w(self, weight, eps, **kw):
        ptr, w = self.lib.ptr, self._vec(weight)
        return self._twice("insar_cross_entropy_w", 2 + 2 * self.nb, 1, lambda dl, out, ws: (
            ptr(self.lg), ptr(self.tg), self.B, self.K, self.HW, IGN, ptr(w), float(eps), ptr(dl), ptr(out), ptr(ws),
            self.lib.stream_ptr()), **kw)

    def focal(self, gamma, alpha, **kw):
        ptr, a = self.lib.ptr, self._vec(alpha)
        return self._twice("insar_focal", 2 + 2 * self.nb, 1, lambda dl, out, ws: (
            ptr(self.lg), ptr(self.tg), self.B, self.K, self.HW, IGN, float(gamma), ptr(a), ptr(dl), ptr(out), ptr(ws),
            self.lib.stream_ptr()), **kw)

    def dice_ce_w(self, weight, eps, gamma, smooth=1.0, wce=1.0, wd=1.0, **kw):
        ptr, w = self.lib.ptr, self._vec(weight)
        g = -1.0 if gamma is None else float(gamma)
        return self._twice("insar_dice_ce_w", 4 + 3 * self.K + self.nb * (3 + 3 * self.K), 3, lambda dl, out, ws: (
            ptr(self.lg), ptr(self.tg), self.B, self.K, self.HW, IGN, float(smooth), float(wce), float(wd), ptr(w), float(eps), g,
            ptr(dl), ptr(out), ptr(ws), self.lib.stream_ptr()), **kw)


def _zero_where_invalid(d, tg, K):
    bad = ~wr.valid(tg, K, IGN)
    assert bool((d[bad.unsqueeze(1).expand_as(d)] == 0).all()), "a gradient element of an invalid pixel is not exactly 0"


def _norm_scale(tg, K, vec):
    """(normaliser in float64, normaliser / largest class weight)."""
    norm = float(wr.normaliser(tg, K, vec, IGN))
    return norm, norm / (1.0 if vec is None else float(vec.max()))


def hold_ce_w(k, family, lg, tg, weight, eps, loss_bound=True):
    out, d, _ = k.ce_w(weight, eps)
    (r, rd), (f, fd) = wr.cross_entropy_w(lg.double(), tg, weight, eps, IGN), wr.cross_entropy_w(lg.float(), tg, weight, eps, IGN)
    what = "ce_w eps=%g" % eps
    if loss_bound:
        _hold(family, what + " loss", float(out[0]), r, f, 1e-6)
    assert math.isfinite(float(out[0]))
    _hold(family, what + " grad*W/wmax", d, rd, fd, 2e-8, scale=_norm_scale(tg, k.K, weight)[1])
    _zero_where_invalid(d, tg, k.K)
    return out, d


def hold_focal(k, family, lg, tg, gamma, alpha):
    out, d, _ = k.focal(gamma, alpha)
    (r, rd), (f, fd) = wr.focal(lg.double(), tg, gamma, alpha, IGN), wr.focal(lg.float(), tg, gamma, alpha, IGN)
    what = "focal g=%g" % gamma
    _hold(family, what + " loss", float(out[0]), r, f, 1e-6)
    n = float(wr.normaliser(tg, k.K, None, IGN))                # focal is normalised by n_valid, whatever alpha is
    _hold(family, what + " grad*n/amax", d, rd, fd, 2e-8, scale=n / (1.0 if alpha is None else float(alpha.max())))
    _zero_where_invalid(d, tg, k.K)
    return out, d


def hold_dice_ce_w(k, family, lg, tg, weight, eps, gamma, wce=1.0, wd=1.0, smooth=1.0, sums=False, loss_bound=True):
    out, d, ws = k.dice_ce_w(weight, eps, gamma, smooth, wce, wd)
    r = wr.dice_ce_w(lg.double(), tg, weight, eps, gamma, smooth, wce, wd, IGN)
    f = wr.dice_ce_w(lg.float(), tg, weight, eps, gamma, smooth, wce, wd, IGN)
    K = k.K
    what = "dice_ce_w %s" % ("focal g=%g" % gamma if gamma is not None else "eps=%g" % eps)
    for i, name in enumerate(("combined", "term", "dice")):
        assert math.isfinite(float(out[i]))
        if loss_bound or i == 2:
            _hold(family, "%s %s" % (what, name), float(out[i]), r[i], f[i], 1e-6)
    counted = weight if gamma is None else None                 # the normaliser: W, or n_valid for focal
    norm = float(wr.normaliser(tg, K, counted, IGN))
    scale = norm / (1.0 if weight is None else float(weight.max()))
    if wce == 0.0:
        _hold(family, what + " grad (Dice alone)", d, r[3], f[3], 2e-8)
    else:
        _hold(family, what + " grad*norm/wmax", d, r[3], f[3], 2e-8, scale=scale)
    _zero_where_invalid(d, tg, K)
    if sums:
        n = int(wr.valid(tg, K, IGN).sum())
        n32 = wr.normaliser(tg, K, counted, IGN, torch.float32)
        _hold(family, what + " ws[0] normaliser / norm", float(ws[0]), norm, float(n32), 1e-6 * norm)
        _hold(family, what + " ws[1] reciprocal * norm", float(ws[1]), 1.0 / norm, float(1.0 / n32), 1e-6 / norm)
        num64, num32 = float(r[1]) * norm, float(f[1].double() * n32.double())
        _hold(family, what + " ws[2] numerator / norm", float(ws[2]), num64, num32, 1e-6 * norm)
        assert float(ws[3]) == float(n)
        s64, s32 = wr.dice_sums(lg.double(), tg, IGN), wr.dice_sums(lg.float(), tg, IGN)
        tot = ws[4:4 + 3 * K].view(3, K)
        _hold(family, what + " ws I totals / n", tot[0], s64[0], s32[0], 1e-6, scale=1.0 / n)
        _hold(family, what + " ws P totals / n", tot[1], s64[1], s32[1], 1e-6, scale=1.0 / n)
        assert torch.equal(tot[2].double(), s64[2])
    return out, d


def _fused_args(mode, K):
    kind, eps, gamma = FUSED_MODES[mode]
    return _wvec(kind, K), eps, gamma


def hold_all(dev, family, lg, tg, offset=0, full=None, sums=True):
    """Every loss entry point on one (logits, target) pair: the whole option grid, or one configuration per entry point (and
    per focal flag of insar_dice_ce_w) when the case is large."""
    B, K, HW = lg.shape
    k = WKernels(dev, lg, tg, offset)
    full = B * HW < LARGE if full is None else full
    for eps, zero in (CE_GRID if full else [(0.1, K >= 3)]):
        hold_ce_w(k, family, lg, tg, class_weights(K, zero), eps)
    for gamma, alpha in (FOCAL_GRID if full else [(2.0, True)]):
        hold_focal(k, family, lg, tg, gamma, class_weights(K) if alpha else None)
    if full:
        for mode in FUSED_MODES:
            for wce, wd in MIXES:
                hold_dice_ce_w(k, family, lg, tg, *_fused_args(mode, K), wce=wce, wd=wd, sums=sums and wce == 0.3)
    else:
        for mode in ("weights_eps", "focal2_alpha"):
            hold_dice_ce_w(k, family, lg, tg, *_fused_args(mode, K), wce=0.3, wd=0.7, sums=sums)
    return k


# ---- grid structure and class counts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 4, 5])
@pytest.mark.parametrize("B,HW", BLOCK_SHAPES)
def test_block_structure(dev, B, HW, K):
    """K = 2, 3, 4: the straight-line lw_main kernels, and the four-pixel Dice+CE kernels where HW % 4 == 0 (the per-pixel ones
    elsewhere); K = 5: the predicated LW_MAXK kernels and the looped fold. (2, 131584) and (3, 87389) are the second trip."""
    lg, tg = block_case(B, K, HW)
    hold_all(dev, "blocks", lg, tg)


@pytest.mark.parametrize("B,HW", [(1, 257), (2, 131584)])
@pytest.mark.parametrize("K", [1, 6, 16])
def test_one_six_sixteen_classes(dev, B, HW, K):
    """The predicated class loops away from K = 5, Dice classes beyond index 4, the looped fold at stride 21 and 51 (and the
    register fold at stride 6). With one class every loss and every gradient element is 0."""
    lg, tg = _logits(B, K, HW, K + B), _targets(B, K, HW, K + 3)
    k = WKernels(dev, lg, tg)
    hold_ce_w(k, "K=1,6,16", lg, tg, class_weights(K, K > 1), 0.1)
    hold_focal(k, "K=1,6,16", lg, tg, 2.0, class_weights(K))
    for mode in ("weights_eps", "focal2_alpha"):
        hold_dice_ce_w(k, "K=1,6,16", lg, tg, *_fused_args(mode, K), wce=0.3, wd=0.7, sums=True)


@pytest.mark.parametrize("B,HW", [(2, 1024), (2, 131584)])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_dice_ce_w_unaligned_fallback(dev, B, HW, K):
    """logits and dlogits one float into a larger buffer, HW % 4 == 0: the LW_MAXK per-pixel kernels with the runtime focal
    flag, both values of it, held to the aligned call's bound."""
    lg, tg = _logits(B, K, HW, 31 + K), _targets(B, K, HW, 32 + K)
    for offset in (0, 1):
        k = WKernels(dev, lg, tg, offset)
        assert k.lg.data_ptr() % 16 == 4 * offset
        for mode in ("weights_eps", "focal2_alpha"):
            hold_dice_ce_w(k, "unaligned" if offset else "aligned", lg, tg, *_fused_args(mode, K), wce=0.3, wd=0.7, sums=True)
    store, dl = k._dl()
    assert dl.data_ptr() % 16 == 4


# ---- validity ------------------------------------------------------------------------------------------------------------------
def _with_stray(tg, K, seed, frac=0.02):
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([K if s is None else s for s in STRAY])
    pick = vals[torch.randint(0, len(vals), tg.shape, generator=g)]
    out = torch.where(torch.rand(tg.shape, generator=g) < frac, pick, tg)
    out[0, 0] = 0
    for i, s in enumerate(vals.tolist()):                      # each of them at least once
        out[0, 1 + i] = s
    return out


def _every_entry_point(k):
    K = k.K
    return [k.ce_w(class_weights(K, True), 0.1), k.focal(2.0, class_weights(K)), k.dice_ce_w(class_weights(K, True), 0.1, None, wce=0.3, wd=0.7),
            k.dice_ce_w(class_weights(K), 0.0, 2.0, wce=0.3, wd=0.7)]


@pytest.mark.parametrize("HW", [1000, 1001])
def test_stray_labels_count_as_ignored(dev, HW):
    """About 2 % of the targets are -1, K, 254 or INT64_MIN: every output and every workspace word is bitwise what the launch
    gives with those pixels set to 255, and the launch is held to the reference, which has the same rule."""
    B, K = 3, 3
    lg, base = _logits(B, K, HW, 81), _targets(B, K, HW, 82)
    tg = _with_stray(base, K, 83)
    stray = ~wr.valid(tg, K, IGN) & (tg != IGN)
    assert int(stray.sum()) >= 30 and {int(v) for v in tg[stray].unique()} == {-1, K, 254, -2 ** 63}
    clean = torch.where(stray, torch.full_like(tg, IGN), tg)
    got, want = _every_entry_point(WKernels(dev, lg, tg)), _every_entry_point(WKernels(dev, lg, clean))
    for a, b in zip(got, want):
        assert _same(a, b)
    hold_all(dev, "stray labels", lg, tg, full=False)


@pytest.mark.parametrize("K,HW", [(2, 1024), (3, 1024), (3, 1001)])
def test_non_finite_logits_under_invalid_pixels(dev, K, HW):
    """NaN, +inf and -inf logits on ignored and on stray-label pixels (HW 1024: the branchless four-pixel kernels, which
    compute every pixel and select; HW 1001 and the lw_main kernels: a branch): loss, gradient and workspace are bitwise those
    of the launch with these logits set to 0, and the gradient there is exactly 0."""
    B = 2
    lg, tg = _logits(B, K, HW, 91), _with_stray(_targets(B, K, HW, 92), K, 93, 0.05)
    bad = ~wr.valid(tg, K, IGN)
    assert int((bad & (tg != IGN)).sum()) >= 30 and int((tg == IGN).sum()) >= 100
    g = torch.Generator().manual_seed(94)
    vals = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0])
    poison = vals[torch.randint(0, 4, (B, K, HW), generator=g)]
    dirty = torch.where(bad.unsqueeze(1) & (poison != 0), poison, lg)
    clean = torch.where(bad.unsqueeze(1), torch.zeros_like(lg), dirty)
    assert int(torch.isnan(dirty).sum()) > 20 and int(torch.isinf(dirty).sum()) > 40 and bool(torch.isfinite(clean).all())
    got, want = _every_entry_point(WKernels(dev, dirty, tg)), _every_entry_point(WKernels(dev, clean, tg))
    for a, b in zip(got, want):
        assert _same(a, b)
        assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())
        _zero_where_invalid(a[1], tg, K)
    hold_all(dev, "non-finite under invalid", dirty, tg, full=False)


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
def test_target_patterns(dev, name, HW):
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
    hold_all(dev, "targets", lg, tg, full=False)


@pytest.mark.parametrize("K,HW", [(2, 1024), (3, 1001), (5, 1024)])
def test_everything_ignored(dev, K, HW):
    """What weighted_loss_ref gives (pinned in test_weighted_loss_ref_host.py): CE_w NaN, focal NaN, Dice 0, combined NaN,
    every gradient element exactly 0. Half of the 'ignored' targets are stray labels."""
    lg = _logits(2, K, HW, 51)
    tg = torch.full((2, HW), IGN)
    tg[1] = K
    k, w = WKernels(dev, lg, tg), class_weights(K)
    out, d, _ = k.ce_w(w, 0.1, expect_written=False)
    assert math.isnan(float(out[0])) and torch.equal(d, torch.zeros_like(d))
    out, d, _ = k.focal(2.0, w, expect_written=False)
    assert math.isnan(float(out[0])) and torch.equal(d, torch.zeros_like(d))
    for eps, gamma in ((0.1, None), (0.0, 2.0)):
        out, d, ws = k.dice_ce_w(w, eps, gamma, wce=0.3, wd=0.7, expect_written=False)
        assert math.isnan(float(out[0])) and math.isnan(float(out[1])) and float(out[2]) == 0.0
        assert torch.equal(d, torch.zeros_like(d))
        assert float(ws[0]) == 0.0 and float(ws[3]) == 0.0 and torch.equal(ws[4:4 + 3 * K], torch.zeros(3 * K))


@pytest.mark.parametrize("K,HW", [(2, 1024), (3, 1001)])
def test_only_zero_weight_classes_valid(dev, K, HW):
    """Every valid pixel carries a class of weight 0: W = 0 and the weighted CE is 0/0 = NaN, as the reference's and torch's.
    Dice does not see the weights and is held as usual; invalid pixels keep a gradient of exactly 0."""
    B = 2
    zero_class = 1
    w = class_weights(K)
    w[zero_class] = 0.0
    lg = _logits(B, K, HW, 55)
    tg = torch.where(_targets(B, K, HW, 56) == IGN, IGN, zero_class)
    assert int((tg == zero_class).sum()) > 100 and int((tg == IGN).sum()) > 100
    k = WKernels(dev, lg, tg)
    out, d, _ = k.ce_w(w, 0.0, expect_written=False)
    assert math.isnan(float(out[0]))
    _zero_where_invalid(d, tg, K)
    out, d, ws = k.dice_ce_w(w, 0.0, None, wce=0.3, wd=0.7, expect_written=False)
    r, f = wr.soft_dice(lg.double(), tg, IGN), wr.soft_dice(lg.float(), tg, IGN)
    assert math.isnan(float(out[0])) and math.isnan(float(out[1])) and float(ws[0]) == 0.0
    _hold("zero-weight only", "dice part", float(out[2]), r[0], f[0], 1e-6)
    _zero_where_invalid(d, tg, K)
    # focal with alpha = 0 on every valid pixel is not degenerate: n_valid > 0, the loss and every gradient element are 0
    out, d, _ = k.focal(2.0, w)
    assert float(out[0]) == 0.0 and torch.equal(d, torch.zeros_like(d))


# ---- extreme logits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0.0, 3e4])
@pytest.mark.parametrize("K,HW", [(2, 1024), (3, 1001)])
def test_saturated_logits(dev, K, HW, base):
    """One class 160 above the others (every logit an integer, so nothing rounds even at 3e4): nothing is inf or NaN. One pixel
    in 64 is labelled against the saturated class, which keeps the unsmoothed losses O(1)."""
    B = 2
    g = torch.Generator().manual_seed(61)
    hot = torch.randint(0, K, (B, HW), generator=g)
    lg = torch.full((B, K, HW), base)
    lg.scatter_(1, hot.unsqueeze(1), base + 160.0)
    tg = torch.where(torch.rand((B, HW), generator=g) < 1.0 / 64, (hot + 1) % K, hot)
    tg = torch.where(torch.rand((B, HW), generator=g) < 0.1, torch.full_like(tg, IGN), tg)
    k, w = WKernels(dev, lg, tg), class_weights(K)
    hold_ce_w(k, "saturated", lg, tg, w, 0.0)
    hold_ce_w(k, "saturated", lg, tg, w, 0.1, loss_bound=False)
    for gamma in (0.0, 0.5, 2.0):
        hold_focal(k, "saturated", lg, tg, gamma, w)
    hold_dice_ce_w(k, "saturated", lg, tg, w, 0.0, None, wce=0.3, wd=0.7)
    hold_dice_ce_w(k, "saturated", lg, tg, w, 0.1, None, wce=0.3, wd=0.7, loss_bound=False)
    hold_dice_ce_w(k, "saturated", lg, tg, w, 0.0, 2.0, wce=0.3, wd=0.7)


@pytest.mark.parametrize("scale", [4.0, 8.0])
@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("entry", ["focal", "dice_ce_w_v4", "dice_ce_w_per_pixel"])
def test_focal_on_confident_pixels(dev, entry, gamma, scale):
    """Logits scaled until hundreds of pixels have q = 1 - p_t below 1e-6: there EVERY gradient entry is held relative to its
    own float64 value (the selection and the gate of tests/test_weighted_loss_gpu.py), through insar_focal and through both
    kernel pairs of insar_dice_ce_w (dice_weight = 0; the per-pixel pair is reached by the one-float offset)."""
    B, K, HW = 3, 2, 1536
    lg, tg = _logits(B, K, HW, 65) * scale, _targets(B, K, HW, 66)
    alpha = torch.tensor([0.75, 0.25])
    k = WKernels(dev, lg, tg, offset=1 if entry == "dice_ce_w_per_pixel" else 0)
    if entry == "focal":
        out, d, _ = k.focal(gamma, alpha)
    else:
        out, d, _ = k.dice_ce_w(alpha, 0.0, gamma, wce=1.0, wd=0.0)
    (r, rd), (f, fd) = wr.focal(lg.double(), tg, gamma, alpha, IGN), wr.focal(lg.float(), tg, gamma, alpha, IGN)
    n = int((tg != IGN).sum())
    fam = "confident x%g" % scale
    _hold(fam, "%s g=%g loss" % (entry, gamma), float(out[1 if entry != "focal" else 0]), r, f, 1e-6)
    _hold(fam, "%s g=%g grad*n/amax" % (entry, gamma), d, rd, fd, 2e-8, scale=n / 0.75)
    l64 = lg.double()
    own = torch.zeros(lg.shape, dtype=torch.bool).scatter_(1, torch.where(tg == IGN, torch.zeros_like(tg), tg).unsqueeze(1), True)
    q = torch.exp(torch.logsumexp(l64.masked_fill(own, float("-inf")), 1) - torch.logsumexp(l64, 1))      # from the other class
    sel = ((tg != IGN) & (q < CONFIDENT_Q)).unsqueeze(1).expand_as(rd) & (rd.abs() > 1e-30)
    assert int(sel.sum()) >= 300, int(sel.sum())
    rel = ((d.double() - rd).abs() / rd.abs())[sel]
    print("LOSSFIG %s | %s g=%g per-entry relative on %d entries with q < %g (min q %.1e) | kernel %.3e | gate %.0e | ratio %.3f"
          % (fam, entry, gamma, int(sel.sum()), CONFIDENT_Q, float(q[tg != IGN].min()), float(rel.max()), CONFIDENT_GATE,
             float(rel.max()) / CONFIDENT_GATE))
    assert float(rel.max()) <= CONFIDENT_GATE


# ---- label histogram -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 16])
@pytest.mark.parametrize("npix", [1, 255, 256, 257, 263168, 262167])
def test_label_hist(dev, npix, K):
    """counts starts at a known non-zero vector between guard words and two successive calls ADD to it; ws, exactly
    (K + 1) * nb int64 between guards, starts as garbage; stray labels are counted nowhere."""
    from insar_unet_ca_amd import _lib
    g = torch.Generator().manual_seed(1000 * K + npix % 997)
    tg = torch.randint(0, K, (npix,), generator=g)
    r = torch.rand((npix,), generator=g)
    tg = torch.where(r < 0.15, torch.full_like(tg, IGN), tg)
    vals = torch.tensor([-1, K, 254, -2 ** 63, K + 1, 2 ** 40])
    tg = torch.where((r > 0.97) | (npix > 16) & (torch.arange(npix) < len(vals)), vals[torch.arange(npix) % len(vals)], tg)
    other = torch.randint(0, K, (npix,), generator=g)
    nb = _lib.call("insar_ce_blocks", npix)
    start = torch.arange(K + 1, dtype=torch.int64) * 1000003 + 17
    store = torch.full((K + 1 + 8,), -77, dtype=torch.int64, device=dev)
    counts = store[4:4 + K + 1]
    counts.copy_(start)
    want = start.clone()
    for t in (tg, other):
        ws_store = torch.full(((K + 1) * nb + 8,), -0x0123456789ABCDEF, dtype=torch.int64, device=dev)
        ws = ws_store[4:4 + (K + 1) * nb]
        td = t.to(dev)
        _lib.call("insar_label_hist", _lib.ptr(td), npix, K, IGN, _lib.ptr(counts), _lib.ptr(ws), _lib.stream_ptr())
        want += wr.label_hist(t, K, IGN)
        assert torch.equal(counts.cpu(), want)
        assert bool((torch.cat([ws_store[:4], ws_store[-4:]]) == -0x0123456789ABCDEF).all()), "wrote outside ws"
        assert bool((ws >= 0).all()) and int(ws.sum()) == int(wr.label_hist(t, K, IGN).sum())       # every partial written
    assert bool((torch.cat([store[:4], store[-4:]]) == -77).all()), "wrote outside counts"
    assert int(wr.label_hist(tg, K, IGN).sum()) < npix or npix <= 16


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    """Every INSAR_FAIL of the four wrappers: the code comes back, insar_last_error names the entry point, and after a
    synchronize the outputs and the workspace still hold the NaN (or the integers) they were filled with."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import ptr
    lib = _lib.load()
    B, K, HW = 1, 2, 16
    lg, tg = torch.zeros(B, 17, HW, device=dev), torch.zeros(B, HW, dtype=torch.int64, device=dev)
    w = torch.ones(17, device=dev)
    dl, out, ws = (torch.full((n,), float("nan"), device=dev) for n in (17 * HW, 3, 256))
    s = _lib.stream_ptr()
    nan, P = float("nan"), dict(lg=ptr(lg), tg=ptr(tg), w=ptr(w), dl=ptr(dl), out=ptr(out), ws=ptr(ws))

    def ce_w(B=B, K=K, HW=HW, eps=0.1, **p):
        a = dict(P, **p)
        return lib.insar_cross_entropy_w(a["lg"], a["tg"], B, K, HW, IGN, a["w"], eps, a["dl"], a["out"], a["ws"], s)

    def focal(B=B, K=K, HW=HW, gamma=2.0, **p):
        a = dict(P, **p)
        return lib.insar_focal(a["lg"], a["tg"], B, K, HW, IGN, gamma, a["w"], a["dl"], a["out"], a["ws"], s)

    def fused(B=B, K=K, HW=HW, eps=0.0, gamma=-1.0, **p):
        a = dict(P, **p)
        return lib.insar_dice_ce_w(a["lg"], a["tg"], B, K, HW, IGN, 1.0, 0.3, 0.7, a["w"], eps, gamma, a["dl"], a["out"], a["ws"], s)

    refused = 0
    for fn, name in ((ce_w, "insar_cross_entropy_w"), (focal, "insar_focal"), (fused, "insar_dice_ce_w")):
        cases = [(dict(**{p: None}), E_ARG) for p in ("lg", "tg", "dl", "out", "ws")]
        cases += [(dict(K=0), E_SHAPE), (dict(K=17), E_SHAPE), (dict(K=-3), E_SHAPE), (dict(B=0), E_SHAPE), (dict(HW=0), E_SHAPE),
                  (dict(B=-1), E_SHAPE), (dict(HW=-4), E_SHAPE)]
        if fn is ce_w:
            cases += [(dict(w=None), E_ARG)]
        if fn is not focal:
            cases += [(dict(eps=v), E_ARG) for v in (-0.1, 1.0, 1.5, nan)]
        if fn is focal:
            cases += [(dict(gamma=v), E_ARG) for v in (-1.0, 64.5, nan)]
        if fn is fused:
            cases += [(dict(gamma=64.5), E_ARG), (dict(gamma=nan), E_ARG), (dict(eps=0.1, gamma=2.0), E_ARG), (dict(eps=0.1, gamma=0.0), E_ARG)]
        for kw, code in cases:
            assert fn(**kw) == code, (name, kw)
            assert name + ":" in lib.insar_last_error().decode(), (name, kw)
            refused += 1
    counts = torch.full((17,), 5, dtype=torch.int64, device=dev)
    iws = torch.full((64,), -9, dtype=torch.int64, device=dev)
    for args, code in (((0, HW, K, IGN, ptr(counts), ptr(iws)), E_ARG), ((ptr(tg), HW, K, IGN, 0, ptr(iws)), E_ARG),
                       ((ptr(tg), HW, K, IGN, ptr(counts), 0), E_ARG), ((ptr(tg), HW, 0, IGN, ptr(counts), ptr(iws)), E_SHAPE),
                       ((ptr(tg), HW, 17, IGN, ptr(counts), ptr(iws)), E_SHAPE), ((ptr(tg), 0, K, IGN, ptr(counts), ptr(iws)), E_SHAPE),
                       ((ptr(tg), -5, K, IGN, ptr(counts), ptr(iws)), E_SHAPE)):
        assert lib.insar_label_hist(*args, s) == code, args
        assert "insar_label_hist:" in lib.insar_last_error().decode()
        refused += 1
    assert refused == 17 + 15 + 20 + 7
    torch.cuda.synchronize()
    assert bool(torch.isnan(dl).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())
    assert bool((counts == 5).all()) and bool((iws == -9).all())
    # the same arguments without the fault are accepted (the table above fails for its stated reason, not for another)
    assert ce_w() == 0 and focal() == 0 and fused() == 0 and fused(gamma=2.0) == 0
    torch.cuda.synchronize()
