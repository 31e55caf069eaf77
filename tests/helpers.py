"""Shared comparison helpers for the parity tests."""
from __future__ import annotations

import numpy as np
import torch

from oracle import closed_form as cf


def fake_abi_result(name: str, a: tuple) -> int:
    """What the mocked C ABI (mock_abi) answers: plausible geometry for the host-side queries, 0 (success) for launches."""
    if name == "insar_igemm_num_mtiles":
        return (a[0] + 127) // 128
    if name == "insar_igemm_tile_rows":
        return 128
    if name == "insar_wgrad_tile":
        return 64
    if name == "insar_wgrad_tile_pair":
        return (64 << 16) | 64
    if name == "insar_conv3x3_small_fwd_rows":
        return 64
    if name == "insar_conv3x3_small_wgrad_blocks":
        return min(a[0] * a[1], 512)
    if name == "insar_conv1x1_out_bwd_blocks":
        return min(a[0] * a[1], 1024)
    if name == "insar_ce_blocks":
        return min((a[0] + 255) // 256, 1024)
    return 0


def mock_abi(monkeypatch, answers=None) -> list:
    """Replace the C ABI under the package's host code, so that plans build and run on CPU tensors without a kernel: `call`
    in every module that launches, the stream pointer, the device check. Returns the list that collects the entry-point
    names in call order. answers: name -> f(*args) for queries that fake_abi_result leaves at 0."""
    from insar_unet_ca_amd import _lib, deeplab, engine, fcn, modules
    calls, answers = [], answers or {}

    def fake_call(name, *a):
        calls.append(name)
        return answers[name](*a) if name in answers else fake_abi_result(name, a)

    for m in (_lib, engine, modules, deeplab, fcn):
        monkeypatch.setattr(m, "call", fake_call, raising=False)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    for m in (modules, deeplab, fcn):
        monkeypatch.setattr(m, "_require_device", lambda x, who: None, raising=False)
    return calls


class LaunchLog(list):
    """(entry point, its arguments, stream the call was issued on) in issue order, as record_calls collects them."""

    def names(self):
        return [n for n, _, _ in self]

    def args(self, name):
        return [a for n, a, _ in self if n == name]

    def count(self, name):
        return sum(1 for n, _, _ in self if n == name)

    def streams(self, name):
        return [s for n, _, s in self if n == name]


def small_ints(args) -> tuple:
    """The integer arguments of a call that are not addresses (flags, extents, nsplit, counts): what two runs with
    different allocations must still agree on."""
    return tuple(a for a in args if isinstance(a, int) and not isinstance(a, bool) and abs(a) < 2 ** 31)


def record_calls(monkeypatch, modules=None) -> LaunchLog:
    """Wrap the real C ABI `call` of the package's launching modules (all of them, or the ones given): every call is
    logged with its arguments and torch's current stream handle, then made. Undone with the monkeypatch."""
    import sys
    from insar_unet_ca_amd import _lib
    log, orig = LaunchLog(), _lib.call

    def recording_call(name, *a):
        log.append((name, a, _lib.stream_ptr()))
        return orig(name, *a)

    recording_call.wraps = orig
    if modules is None:      # every module that launches: it holds the ABI's `call`, or an earlier recorder of this kind
        modules = [m for k, m in list(sys.modules.items()) if k.startswith("insar_unet_ca_amd.") and m is not _lib
                   and (getattr(m, "call", None) is orig or getattr(getattr(m, "call", None), "wraps", None) is orig)]
    assert modules
    for m in modules:
        monkeypatch.setattr(m, "call", recording_call)
    return log


def to_np(t):
    if isinstance(t, torch.Tensor):
        return t.detach().double().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def max_rel(a, b) -> float:
    """max |a-b| / max|b| (the 'max-rel' figure of SURVEY §8d)."""
    a, b = to_np(a), to_np(b)
    den = np.abs(b).max()
    if den == 0:
        return float(np.abs(a).max())
    return float(np.abs(a - b).max() / den)


def check_summary(store, prefix: str, t, rtol: float, what: str = "") -> None:
    """Compare tensor `t` against a fixture written by oracle.gen_golden.summarize()."""
    a = to_np(t).reshape(-1)
    absmax = float(store[f"{prefix}/absmax"])
    scale = max(absmax, 1e-30)
    idx = cf.sample_indices(a.size, 64)
    exp = store[f"{prefix}/samples"].astype(np.float64)
    err = np.abs(a[idx] - exp).max() / scale
    assert err <= rtol, f"{what or prefix}: sampled max-rel {err:.3e} > {rtol:.1e}"
    nrm = float(store[f"{prefix}/norm"])
    got = float(np.sqrt((a * a).sum()))
    assert abs(got - nrm) <= rtol * max(nrm, 1e-30) * 4 + 1e-12, \
        f"{what or prefix}: norm {got:.6e} vs {nrm:.6e}"
    key = f"{prefix}/full"
    if key in store.files:
        full = store[key].astype(np.float64).reshape(-1)
        err = np.abs(a - full).max() / scale
        assert err <= rtol, f"{what or prefix}: full max-rel {err:.3e} > {rtol:.1e}"


def check_grad_summary(store, prefix: str, t, rtol: float, outlier_frac: float = 2e-3, what: str = "") -> None:
    """Gradient comparison that tolerates isolated ReLU-mask flips: a pre-activation that sits within
    rounding of 0 may get a different mask in two fp32 implementations, which changes ONE element of a
    BN/bias gradient (or a thin slice of a weight gradient) by O(1) while everything else agrees.
    Rules: the norm agrees to 4*rtol; at most one of the 64 sampled elements may miss rtol; for tensors
    stored whole, at most `outlier_frac` of the elements (and at least one) may miss rtol."""
    a = to_np(t).reshape(-1)
    scale = max(float(store[f"{prefix}/absmax"]), 1e-30)
    idx = cf.sample_indices(a.size, 64)
    exp = store[f"{prefix}/samples"].astype(np.float64)
    bad = int((np.abs(a[idx] - exp) / scale > rtol).sum())
    assert bad <= 1, f"{what or prefix}: {bad} of {len(idx)} sampled elements off by more than {rtol:.1e}"
    nrm = float(store[f"{prefix}/norm"])
    got = float(np.sqrt((a * a).sum()))
    assert abs(got - nrm) <= 4 * rtol * max(nrm, 1e-30) + 1e-12, f"{what or prefix}: norm {got:.6e} vs {nrm:.6e}"
    key = f"{prefix}/full"
    if key in store.files:
        full = store[key].astype(np.float64).reshape(-1)
        nbad = int((np.abs(a - full) / scale > rtol).sum())
        assert nbad <= max(1, int(outlier_frac * a.size)), \
            f"{what or prefix}: {nbad} of {a.size} elements off by more than {rtol:.1e}"
