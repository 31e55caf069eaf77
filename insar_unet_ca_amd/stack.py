"""Detections through a stack of dates on the device (csrc/stack.hip): what a user does today with `mask.cpu()` per date and a
numpy loop, without the copies. `warp_raster` / `grid_matrix` put every date on one pixel grid; a `DetectionStack` then holds
up to 256 of them as two bit-plane tensors,

    hit, valid   int64 [words, H, W]       date t is bit t & 63 of plane t >> 6, T = 64 * words dates

A date is valid at a pixel where it was observed (the class map is not `ignore`, the optional validity map is not 0) and a hit
where it is valid, its class is in the class set and its confidence reaches `min_conf`. `summary` answers the per-pixel
questions (how often, since when, how long without a break, and the persistence rule), `site_series` the per-site ones (how
many pixels of each label were hits / observed at each date), `follow_sites` chains them through `label_regions`.

Everything the device computes is an integer and defined by one scan over the dates that SKIPS unobserved ones: a missing
observation neither breaks nor extends a run. Nothing is read back before the series table."""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_on_device, is_int, query_bytes, read_back
from .regions import DEFAULT_MAX_REGIONS, label_regions

MAX_WORDS = 4
MAX_DATES = 64 * MAX_WORDS
SUMMARY_PLANES = ("n_valid", "n_hit", "longest_run", "run_start", "first_hit", "last_hit", "known", "persistent")
_PLANE_DTYPE = {p: (torch.uint8 if p in ("known", "persistent") else torch.int16) for p in SUMMARY_PLANES}
SERIES_HEADER = 4                                                 # int32 words before the first row of the table


def class_words(classes) -> tuple:
    """The class set as four 64-bit words: class c is bit c & 63 of word c >> 6. `classes`: one class or an iterable."""
    cs = [classes] if is_int(classes) else classes
    try:
        cs = list(cs)
    except TypeError:
        raise InsarError(f"classes={classes!r}: a class or an iterable of classes in 0..255") from None
    if not cs or not all(is_int(c) and 0 <= c <= 255 for c in cs):
        raise InsarError(f"classes={classes!r}: at least one class, each an integer in 0..255")
    w = [0, 0, 0, 0]
    for c in cs:
        w[int(c) >> 6] |= 1 << (int(c) & 63)
    return tuple(w)


def _check_fraction(name: str, f) -> tuple:
    try:
        num, den = f
    except (TypeError, ValueError):
        raise InsarError(f"{name}={f!r}: two integers (num, den)") from None
    if not (is_int(num) and is_int(den)) or den < 1 or den >= 1 << 31 or not 0 <= num <= den:
        raise InsarError(f"{name}={f!r}: integers with 0 <= num <= den, 1 <= den < 2^31")
    return int(num), int(den)


def _check_window(T: int, n_dates: int, t0, t1) -> tuple:
    t1 = n_dates if t1 is None else t1
    if not (is_int(t0) and is_int(t1)) or not 0 <= t0 <= t1 <= T:
        raise InsarError(f"window t0={t0!r}, t1={t1!r}: integers with 0 <= t0 <= t1 <= {T} dates")
    return int(t0), int(t1)


def _check_caps(who: str, max_regions, count=None) -> None:
    check_int(who, "max_regions", max_regions, 1, 1 << 24, integral_floats=False)
    if count is not None:
        check_int(who, "count", count, 0, max_regions, integral_floats=False, expect=f"an integer in 0..max_regions={max_regions}")


def series_bytes(max_regions: int = DEFAULT_MAX_REGIONS, n_dates: int = 64) -> int:
    """Bytes of the series table for max_regions rows of n_dates dates. Host arithmetic only."""
    return query_bytes("insar_stack_series_bytes", max_regions, n_dates, outputs=1)


class DetectionStack:
    """The bit planes of one H x W grid and the number of dates pushed so far (kept on the host: nothing is read back).

        st = DetectionStack(H, W, device, words=1)            # 64 dates per word, up to 4 words
        st.push(mask, conf=conf, min_conf=0.6)                # appends at st.n_dates; [n, H, W] pushes n dates in one launch
        st.push(mask, t=3)                                    # overwrites date 3, every other bit keeps its value
        st.shift(1)                                           # drops the oldest date: a monitoring job adds one date per pass
        planes = st.summary(min_hits=3, min_run=2, min_fraction=(1, 2))
    """

    def __init__(self, H: int, W: int, device, words: int = 1):
        if not (is_int(H) and is_int(W)) or H < 1 or W < 1 or H * W >= 1 << 31:
            raise InsarError(f"DetectionStack: grid {H!r} x {W!r}: integers with H, W >= 1 and H * W < 2^31")
        self.H, self.W, self.words = int(H), int(W), check_int("DetectionStack", "words", words, 1, MAX_WORDS, integral_floats=False)
        self.device = torch.device(device)
        self.hit = torch.zeros(self.words, self.H, self.W, dtype=torch.int64, device=self.device)
        self.valid = torch.zeros(self.words, self.H, self.W, dtype=torch.int64, device=self.device)
        self.n_dates = 0

    @property
    def T(self) -> int:
        return 64 * self.words

    def _on_device(self, who: str) -> None:
        check_on_device(who, "the stack", self.hit)

    def _plane_input(self, who: str, name: str, x, dtype, n: Optional[int]):
        if not isinstance(x, torch.Tensor):
            raise InsarError(f"{who}: {name} must be a torch tensor, got {type(x).__name__}")
        if x.dtype != dtype:
            raise InsarError(f"{who}: {name} dtype {x.dtype}: {dtype}")
        shape = tuple(x.shape)
        ok = shape == (self.H, self.W) or (len(shape) == 3 and shape[1:] == (self.H, self.W) and shape[0] >= 1)
        if not ok or (n is not None and (1 if len(shape) == 2 else shape[0]) != n):
            want = f"[{self.H}, {self.W}] or [n, {self.H}, {self.W}]" if n is None else f"{n} dates of [{self.H}, {self.W}], as the mask"
            raise InsarError(f"{who}: {name} shape {shape}: {want}")
        if not x.is_contiguous():
            raise InsarError(f"{who}: {name} must be contiguous")
        return 1 if len(shape) == 2 else shape[0]

    def push(self, mask: torch.Tensor, t: Optional[int] = None, *, valid: Optional[torch.Tensor] = None,
             conf: Optional[torch.Tensor] = None, min_conf: float = 0.0, classes=1, ignore: Optional[int] = 255) -> int:
        """Dates t .. t + n - 1 <- the n class maps of `mask` (uint8 [H, W] or [n, H, W]); t=None appends at n_dates. Exactly
        those bits are written. `valid` uint8, 0 = not observed; `conf` float32, a hit needs conf >= min_conf (NaN: valid, no
        hit); `classes` one class or several in 0..255; `ignore` a class value that means not observed (None: none). One launch.
        Returns t."""
        who = "DetectionStack.push"
        n = self._plane_input(who, "mask", mask, torch.uint8, None)
        if valid is not None:
            self._plane_input(who, "valid", valid, torch.uint8, n)
        if conf is not None:
            self._plane_input(who, "conf", conf, torch.float32, n)
        t = self.n_dates if t is None else t
        if not is_int(t) or t < 0 or t + n > self.T:
            raise InsarError(f"{who}: dates {t!r}..{t + n - 1 if is_int(t) else '?'} beyond the stack's 0..{self.T - 1} ({self.words} words)")
        cw = class_words(classes)
        ignore = check_int(who, "ignore", -1 if ignore is None else ignore, -1, 255, integral_floats=False,
                           expect="a class value in 0..255, or None")
        try:
            mc = float(np.float32(min_conf))
        except (TypeError, ValueError):
            mc = math.nan
        if not math.isfinite(mc):
            raise InsarError(f"min_conf={min_conf!r}: a finite number")
        self._on_device(who)
        for name, x in (("mask", mask), ("valid", valid), ("conf", conf)):
            if x is not None:
                check_on_device(who, name, x, like=self.hit)
        with torch.cuda.device(self.hit.device):
            call("insar_stack_push", ptr(mask), ptr(valid), ptr(conf), mc, cw[0], cw[1], cw[2], cw[3], int(ignore), n, int(t), self.words,
                 self.H, self.W, ptr(self.hit), ptr(self.valid), _lib.stream_ptr())
        self.n_dates = max(self.n_dates, int(t) + n)
        return int(t)

    def shift(self, k: int) -> None:
        """Drop the k oldest dates in place: date t takes date t + k, the top k dates become unobserved. k >= T clears."""
        check_int("DetectionStack.shift", "k", k, 0, (1 << 31) - 1, integral_floats=False)
        self._on_device("DetectionStack.shift")
        with torch.cuda.device(self.hit.device):
            call("insar_stack_shift", ptr(self.hit), ptr(self.valid), self.words, self.H, self.W, int(k), _lib.stream_ptr())
        self.n_dates = max(0, self.n_dates - int(k))

    def summary(self, t0: int = 0, t1: Optional[int] = None, *, min_hits: int = 1, min_run: int = 1, min_valid: int = 1,
                min_fraction=(0, 1), want: Sequence[str] = SUMMARY_PLANES) -> Dict[str, torch.Tensor]:
        """The planes named in `want` over the dates t0 .. t1 - 1 (t1=None: n_dates), as fresh device tensors [H, W]:
        n_valid, n_hit, longest_run, run_start, first_hit, last_hit (int16; dates are indices into the stack, -1: none),
        known = n_valid >= min_valid and persistent = known and n_hit >= min_hits and longest_run >= min_run and
        n_hit * den >= num * n_valid with min_fraction = (num, den) (uint8). One launch; planes not asked for are not
        allocated."""
        t0, t1 = _check_window(self.T, self.n_dates, t0, t1)
        for name, v in (("min_hits", min_hits), ("min_run", min_run), ("min_valid", min_valid)):
            check_int("DetectionStack.summary", name, v, 0, 32767, integral_floats=False)
        num, den = _check_fraction("min_fraction", min_fraction)
        want = [want] if isinstance(want, str) else list(want)
        if not want or any(p not in SUMMARY_PLANES for p in want) or len(set(want)) != len(want):
            raise InsarError(f"want={want!r}: at least one of {SUMMARY_PLANES}, each once")
        self._on_device("DetectionStack.summary")
        out = {p: torch.empty(self.H, self.W, dtype=_PLANE_DTYPE[p], device=self.hit.device) for p in want}
        with torch.cuda.device(self.hit.device):
            call("insar_stack_summary", ptr(self.hit), ptr(self.valid), self.words, self.H, self.W, t0, t1, int(min_hits), int(min_run),
                 int(min_valid), num, den, *[ptr(out.get(p)) for p in SUMMARY_PLANES], _lib.stream_ptr())
        return out

    def state_dict(self) -> dict:
        return {"hit": self.hit, "valid": self.valid, "n_dates": self.n_dates, "words": self.words, "shape": (self.H, self.W)}

    def load_state_dict(self, state: dict) -> None:
        """The planes are copied into this stack's own tensors (from the host or any device)."""
        try:
            hit, valid, n_dates = state["hit"], state["valid"], state["n_dates"]
        except (KeyError, TypeError):
            raise InsarError("load_state_dict: a dict with hit, valid and n_dates") from None
        want = (self.words, self.H, self.W)
        for name, x in (("hit", hit), ("valid", valid)):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.int64 or tuple(x.shape) != want:
                raise InsarError(f"load_state_dict: {name} must be an int64 tensor {want}, got "
                                 f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
        check_int("load_state_dict", "n_dates", n_dates, 0, self.T, integral_floats=False)
        self.hit.copy_(hit)
        self.valid.copy_(valid)
        self.n_dates = int(n_dates)


class StackScratch(Scratch):
    """The device series table of one (max_regions, n_dates) and the pinned host copy it is read back into. Nothing in it
    has to survive between calls. `table`: a contiguous uint8 device tensor of exactly `series_bytes(...)` bytes, 16-byte
    aligned, to use instead of a fresh allocation."""
    KEY = ("max_regions", "n_dates")

    def __init__(self, device: torch.device, max_regions: int = DEFAULT_MAX_REGIONS, n_dates: int = 64,
                 table: Optional[torch.Tensor] = None):
        tb = series_bytes(max_regions, n_dates)
        super().__init__((max_regions, n_dates), device, table=self.adopt_table("StackScratch", table, tb), host=tb)


def scan_runs(hit: np.ndarray, valid: np.ndarray, t0: int = 0) -> Dict[str, np.ndarray]:
    """The scan of the device summary on host arrays bool [N, nt]: dates with valid = 0 are skipped. Returns int64 [N] n_valid,
    n_hit, longest_run, run_start, first_hit, last_hit; dates are t0 + column, -1: none."""
    hit = np.asarray(hit, dtype=bool) & np.asarray(valid, dtype=bool)
    valid = np.asarray(valid, dtype=bool)
    N, nt = hit.shape
    z = lambda v: np.full(N, v, dtype=np.int64)
    best, best_start, cur, cur_start, first, last = z(0), z(-1), z(0), z(-1), z(-1), z(-1)
    for i in range(nt):
        h, miss = hit[:, i], valid[:, i] & ~hit[:, i]
        cur_start = np.where(h & (cur == 0), t0 + i, cur_start)
        cur = cur + h
        better = cur > best                                        # strictly: the earliest run wins a tie
        best, best_start = np.where(better, cur, best), np.where(better, cur_start, best_start)
        cur, cur_start = np.where(miss, 0, cur), np.where(miss, -1, cur_start)
        first = np.where(h & (first < 0), t0 + i, first)
        last = np.where(h, t0 + i, last)
    return {"n_valid": valid.sum(axis=1).astype(np.int64), "n_hit": hit.sum(axis=1).astype(np.int64), "longest_run": best,
            "run_start": best_start, "first_hit": first, "last_hit": last}


def series_from_table(raw: np.ndarray, *, max_regions: int, n_dates: int, count: Optional[int], t0: int = 0,
                      active_fraction=(1, 2)) -> Dict[str, object]:
    """The result of `site_series` (fresh arrays) from the raw bytes of a series table, or of its first `count` rows."""
    num, den = _check_fraction("active_fraction", active_fraction)
    N = int(max_regions if count is None else count)
    row = 1 + 2 * n_dates
    words = raw[:4 * (SERIES_HEADER + N * row)].view("<i4")
    rows = words[SERIES_HEADER:].reshape(N, row).astype(np.int64)
    area, hits, valids = rows[:, 0].copy(), rows[:, 1:1 + n_dates].copy(), rows[:, 1 + n_dates:].copy()
    observed = 2 * valids >= area[:, None]
    active = (valids > 0) & (hits * den >= num * valids)
    s = scan_runs(active, observed, t0)
    return {"area": area, "hits": hits, "valids": valids, "out_of_range": int(words[0]), "observed": observed, "active": active,
            "onset": s["first_hit"], "last_active": s["last_hit"], "n_active": s["n_hit"], "longest_active_run": s["longest_run"],
            "t0": int(t0), "t1": int(t0) + int(n_dates)}


def _check_series_args(stack, labels, max_regions, count, t0, t1, active_fraction, scratch):
    who = "site_series"
    if not isinstance(stack, DetectionStack):
        raise InsarError(f"{who}: stack must be a DetectionStack, got {type(stack).__name__}")
    if not isinstance(labels, torch.Tensor):
        raise InsarError(f"{who}: labels must be a torch tensor, got {type(labels).__name__}")
    if labels.dtype != torch.int32 or tuple(labels.shape) != (stack.H, stack.W):
        raise InsarError(f"{who}: labels must be an int32 [{stack.H}, {stack.W}] tensor, got {labels.dtype} {tuple(labels.shape)}")
    if not labels.is_contiguous():
        raise InsarError(f"{who}: labels must be contiguous")
    _check_caps(who, max_regions, count)
    t0, t1 = _check_window(stack.T, stack.n_dates, t0, t1)
    _check_fraction("active_fraction", active_fraction)
    key = (int(max_regions), t1 - t0)
    if scratch is not None:
        StackScratch.check(who, scratch, key, table_bytes=series_bytes(*key))
    stack._on_device(who)
    check_on_device(who, "labels", labels, like=stack.hit)
    if scratch is not None and scratch.table.device != labels.device:
        raise InsarError(f"{who}: the scratch lives on {scratch.table.device}, labels on {labels.device}")
    return t0, t1


def site_series(stack: DetectionStack, labels: torch.Tensor, *, max_regions: int = DEFAULT_MAX_REGIONS, count: Optional[int] = None,
                t0: int = 0, t1: Optional[int] = None, active_fraction=(1, 2), scratch: Optional[StackScratch] = None) -> dict:
    """Per label of a device label map (`label_regions`, `rasterise_polygons(int32)`, ...) and per date of the window:

        s = site_series(stack, det["labels"], count=det["count"])          # rows aligned with det["regions"]["id"]
        s["area"] int64 [N]      s["hits"], s["valids"] int64 [N, t1 - t0]  pixels of the label that are hits / observed
        s["out_of_range"]        pixels whose label exceeds max_regions
        s["observed"] = 2 valids >= area        s["active"] = valids > 0 and hits * den >= num * valids      bool [N, t1 - t0]
        s["onset"], s["last_active"] (dates, -1: never), s["n_active"], s["longest_active_run"]   int64 [N]

    with active_fraction = (num, den); the per-site fields come from the pixel scan's rule with `observed` as the valid bit:
    a date at which less than half of the site was observed neither breaks nor extends a run. N is `count` if given, else
    max_regions. Two launches and ONE read-back, of `count` rows when given."""
    t0, t1 = _check_series_args(stack, labels, max_regions, count, t0, t1, active_fraction, scratch)
    nt, max_regions = t1 - t0, int(max_regions)
    if scratch is None:
        scratch = StackScratch(labels.device, max_regions, nt)
    nbytes = scratch.table.numel() if count is None else 4 * (SERIES_HEADER + int(count) * (1 + 2 * nt))
    with torch.cuda.device(labels.device):
        s = _lib.stream_ptr()
        call("insar_stack_series_clear", ptr(scratch.table), max_regions, nt, s)
        call("insar_stack_series", ptr(stack.hit), ptr(stack.valid), stack.words, ptr(labels), stack.H, stack.W, t0, t1, max_regions,
             ptr(scratch.table), s)
        raw = read_back(scratch.host, scratch.table, nbytes)
    return series_from_table(raw, max_regions=max_regions, n_dates=nt, count=count, t0=t0,
                             active_fraction=active_fraction)


def follow_sites(stack: DetectionStack, *, connectivity: int = 8, min_area: int = 1, max_regions: int = DEFAULT_MAX_REGIONS,
                 active_fraction=(1, 2), t0: int = 0, t1: Optional[int] = None, want: Iterable[str] = SUMMARY_PLANES,
                 region_scratch=None, scratch: Optional[StackScratch] = None, **rule) -> dict:
    """`stack.summary(t0, t1, **rule)`, `label_regions` of its persistent map, `site_series` of those labels:

        out = follow_sites(stack, min_hits=3, min_run=2, min_fraction=(1, 2), min_area=16)
        out["labels"], out["mask"], out["count"], out["regions"]      as label_regions returns them
        out["area"], out["hits"], out["onset"], ...                   as site_series returns them, rows aligned with regions["id"]
        out["summary"]                                                the planes of `want` (persistent always among them)

    The sites are the connected regions of the pixels that are persistent over the window: a site that moves across the
    dates is followed only where its footprints overlap for long enough to meet the rule."""
    if not isinstance(stack, DetectionStack):
        raise InsarError(f"follow_sites: stack must be a DetectionStack, got {type(stack).__name__}")
    want = [want] if isinstance(want, str) else list(want)
    if "persistent" not in want:
        want.append("persistent")
    _check_caps("follow_sites", max_regions)
    _check_fraction("active_fraction", active_fraction)
    planes = stack.summary(t0, t1, want=want, **rule)
    reg = label_regions(planes["persistent"], connectivity=connectivity, min_area=min_area, max_regions=max_regions,
                        scratch=region_scratch)
    series = site_series(stack, reg["labels"], max_regions=max_regions, count=reg["count"], t0=t0, t1=t1,
                         active_fraction=active_fraction, scratch=scratch)
    return {**reg, **series, "summary": planes}
