"""Sieving class maps on the device (csrc/sieve.hip: insar_sieve_remap / _pairs / _rounds / _apply on top of the
insar_regions_* phases): regions smaller than a per-class threshold are absorbed by their largest neighbour, whatever class
that neighbour has, so specks vanish and holes fill by one rule. `label_regions(min_area=)` only drops small foreground regions;
`sieve_regions` cleans the class map itself, and everything after it (regions, outlines, statistics, scores, stacks, crops) sees
the cleaned map. `region_adjacency` is the table underneath: which regions of a label map touch, along how many pixel edges.
`ScenePredictor.detect(..., sieve={1: 64, 0: 16})` sieves what it predicted.

The rule, in integers (tests/sieve_ref.py restates it in numpy; DESIGN.md, "Sieving class maps"): the input regions are the
connected components over ALL classes, class 0 included, with the given connectivity; void pixels belong to no region; regions
are numbered 1..N by ascending smallest row-major pixel index (`label_regions`'s order). Two regions are adjacent if a pixel of
one is a horizontal or vertical neighbour of a pixel of the other (always 4-adjacency; void and the scene edge give nothing).
Pieces start as the regions: a piece's id and class are those of its root region, its area the sum over its members, and
key(u) = (area[u], -id[u]). Rounds are synchronous on a snapshot: every piece u with area[u] < T[cls[u]] and a neighbouring
piece takes best(u), the neighbouring piece with the greatest key, and merges into it unless best(best(u)) == u and
key(u) > key(best(u)); pointers are compressed, areas added into the roots, and the next round sees the merged pieces. A round
that merges nothing ends the loop. At the fixed point no piece below its class threshold has a neighbour; pieces enclosed only
by void or the scene edge stay as they are. Sieving the output again changes nothing.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import MERGE_CTRL_WORDS as CTRL_WORDS  # noqa: F401  pairs, overflow, regions, class-255 pixels, changed pixels, absorbed, 2 spare
from ._scene import MERGE_ROUNDS_PER_READ as ROUNDS_PER_READ  # noqa: F401  (the tools read them from here)
from ._scene import Scratch, check_int, check_map, check_on_device, merge_rounds, pinned, query_bytes, read_back
from .regions import DEFAULT_MAX_REGIONS, RegionScratch
from .regions import _launch as _label_launch

DEFAULT_MAX_PAIRS = 1 << 20
MAX_PAIRS = 1 << 24
MAX_ROUNDS = 4096
MAX_REGIONS = 1 << 30
MAX_LABEL = (1 << 31) - 1

# a record of the pair list; the 16-byte header in front of it is {n_pairs, overflow, 0, 0} as int32
PAIR_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("edges", "<i8")])
assert PAIR_DTYPE.itemsize == 16


def scratch_bytes(H: int, W: int, max_regions: int = DEFAULT_MAX_REGIONS, max_pairs: int = DEFAULT_MAX_PAIRS, max_rounds: int = 64):
    """(scratch bytes, offset of the control words, their bytes, offset of the pair list's header). Host arithmetic only."""
    return query_bytes("insar_sieve_scratch_bytes", H, W, max_regions, max_pairs, max_rounds, outputs=4)


class SieveScratch(Scratch):
    """The device buffers of one (H, W, max_regions, max_pairs, max_rounds): the remapped map, the piece state, the pair table
    and list, the control words with their pinned host copy, and a RegionScratch for the labelling (made on first use, as is
    the host copy of the pair list that `region_adjacency` reads). Nothing in them has to survive between calls."""
    KEY, DEVICE_AT = ("H", "W", "max_regions", "max_pairs", "max_rounds"), 2

    def __init__(self, H: int, W: int, device, max_regions: int = DEFAULT_MAX_REGIONS, max_pairs: int = DEFAULT_MAX_PAIRS,
                 max_rounds: int = 64):
        sb, off, cb, poff = scratch_bytes(H, W, max_regions, max_pairs, max_rounds)
        super().__init__((H, W, max_regions, max_pairs, max_rounds), device, scratch=sb)
        self.remap = self.scratch[:H * W].view(H, W)
        self.ctrl, self.ctrl_host = self.scratch[off:off + cb], pinned(cb)
        self.state = self.scratch[off:off + cb + 4 * (max_regions + 1)]      # the control words and the roots behind them
        self.pairs = self.scratch[poff:poff + 16 * (1 + max_pairs)]
        self.thresholds = torch.zeros(256, dtype=torch.int32, device=device)
        self.regions = self.state_host = self.pairs_host = None


def threshold_table(min_area, who: str = "sieve_regions") -> np.ndarray:
    """The 256-entry int32 table T of `min_area`: an int (every class), a {class: int} dict (missing classes 0) or a sequence
    indexed by class (the rest 0). T[c] = 0: regions of class c are never absorbed."""
    T = np.zeros(256, dtype=np.int32)
    expect = "an integer in 0..2^31-1"
    if isinstance(min_area, dict):
        for c, t in min_area.items():
            c = check_int(who, "min_area: class", c, 0, 255, integral_floats=False)
            T[c] = check_int(who, f"min_area[{c}]", t, 0, MAX_LABEL, integral_floats=True, expect=expect)
    elif isinstance(min_area, (list, tuple, np.ndarray)):
        if np.ndim(min_area) != 1 or len(min_area) > 256:
            raise InsarError(f"{who}: min_area: a sequence indexed by class has at most 256 entries, got shape {np.shape(min_area)}")
        for c, t in enumerate(min_area):
            T[c] = check_int(who, f"min_area[{c}]", t.item() if isinstance(t, np.generic) else t, 0, MAX_LABEL,
                             integral_floats=True, expect=expect)
    elif isinstance(min_area, (int, float, np.integer, np.floating)) and not isinstance(min_area, bool):
        T[:] = check_int(who, "min_area", min_area, 0, MAX_LABEL, integral_floats=True, expect=expect)
    else:
        raise InsarError(f"{who}: min_area={min_area!r}: an integer, a {{class: int}} dict or a sequence indexed by class")
    return T


def _check_caps(who: str, max_regions, max_pairs, max_rounds):
    return (check_int(who, "max_regions", max_regions, 1, MAX_REGIONS, integral_floats=True),
            check_int(who, "max_pairs", max_pairs, 1, MAX_PAIRS, integral_floats=True),
            check_int(who, "max_rounds", max_rounds, 1, MAX_ROUNDS, integral_floats=True))


def _check_shape(who: str, name: str, m) -> tuple:
    H, W = m.shape
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise InsarError(f"{who}: {name} {H} x {W}: need H, W >= 1 and H * W < 2^31")
    return int(H), int(W)


def region_adjacency(labels: torch.Tensor, *, max_pairs: int = DEFAULT_MAX_PAIRS, scratch: Optional[SieveScratch] = None) -> dict:
    """Which regions of a device label map (int32 [H, W]; values <= 0 are no region, any positive ids) touch.

        adj = region_adjacency(det["labels"])
        adj["a"], adj["b"]  int32 [P]  the pairs, a < b, sorted by (a, b)      adj["edges"]  int64 [P]  shared pixel edges
        adj["count"]        P

    Every horizontally or vertically adjacent pixel pair with two different positive labels counts once under (min, max): always
    4-adjacency. Works on `label_regions` and `split_regions` outputs alike. More than `max_pairs` pairs raise InsarError.
    3 launches on the current stream and ONE read-back. `scratch`: a SieveScratch of this H, W and max_pairs to reuse."""
    who = "region_adjacency"
    check_map(who, "labels", labels, (torch.int32,))
    H, W = _check_shape(who, "labels", labels)
    max_pairs = check_int(who, "max_pairs", max_pairs, 1, MAX_PAIRS, integral_floats=True)
    if scratch is not None:
        if not isinstance(scratch, SieveScratch):
            raise InsarError(f"{who}: scratch must be a SieveScratch, got {type(scratch).__name__}")
        if (scratch.H, scratch.W, scratch.max_pairs) != (H, W, max_pairs) or scratch.device != labels.device:
            raise InsarError(f"{who}: scratch of {scratch.H} x {scratch.W}, max_pairs={scratch.max_pairs} on {scratch.device} for "
                             f"{H} x {W}, max_pairs={max_pairs} on {labels.device}")
    check_on_device(who, "labels", labels)
    if scratch is None:
        scratch = SieveScratch(H, W, labels.device, 1, max_pairs, 1)
    if scratch.pairs_host is None:
        scratch.pairs_host = pinned(16 * (1 + max_pairs))
    with torch.cuda.device(labels.device):
        call("insar_sieve_pairs", ptr(labels), H, W, MAX_LABEL, scratch.max_regions, max_pairs, scratch.max_rounds,
             ptr(scratch.scratch), _lib.stream_ptr())
        raw = read_back(scratch.pairs_host, scratch.pairs)
    n, overflow = (int(v) for v in raw[:8].view(np.int32))
    if overflow or n > max_pairs:
        raise InsarError(f"{who}: {'more than ' if overflow else ''}{n} adjacent region pairs exceed max_pairs={max_pairs}: "
                         f"raise max_pairs")
    rec = raw[16:16 * (1 + n)].view(PAIR_DTYPE)
    order = np.lexsort((rec["b"], rec["a"]))
    return {"a": rec["a"][order].astype(np.int32), "b": rec["b"][order].astype(np.int32), "edges": rec["edges"][order].astype(np.int64),
            "count": n}


def _check_args(mask, min_area, connectivity, void_value, max_regions, max_pairs, max_rounds, return_changed, scratch):
    """(H, W, T, void, caps): everything but the launches; the devices are looked at last."""
    who = "sieve_regions"
    check_map(who, "mask", mask, (torch.uint8,))
    H, W = _check_shape(who, "mask", mask)
    T = threshold_table(min_area, who)
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise InsarError(f"{who}: connectivity={connectivity!r}: 4 or 8")
    void = -1 if void_value is None else check_int(who, "void_value", void_value, 0, 255, integral_floats=False,
                                                   expect="an integer in 0..255, or None")
    caps = _check_caps(who, max_regions, max_pairs, max_rounds)
    if not isinstance(return_changed, (bool, np.bool_)):
        raise InsarError(f"{who}: return_changed={return_changed!r}: True or False")
    if scratch is not None:
        SieveScratch.check(who, scratch, (H, W) + caps, mask.device)
    check_on_device(who, "mask", mask)
    return H, W, T, void, caps


def sieve_regions(mask: torch.Tensor, *, min_area, connectivity: int = 8, void_value: Optional[int] = 255,
                  max_regions: int = DEFAULT_MAX_REGIONS, max_pairs: int = DEFAULT_MAX_PAIRS, max_rounds: int = 64,
                  return_changed: bool = False, scratch: Optional[SieveScratch] = None) -> dict:
    """A device class map (uint8 [H, W]) with its small regions absorbed by their largest neighbours.

        out = sieve_regions(mask, min_area={1: 64, 0: 16})       # drop sites under 64 px, fill holes under 16 px
        out["mask"]       uint8 [H, W], a fresh tensor            out["regions_in"]  N, the regions of the input map
        out["absorbed"]   input regions that were absorbed        out["changed_pixels"]  pixels whose class changed
        out["rounds"]     rounds that merged something            out["converged"]  whether a round that merged nothing was
        out["labels_in"]  int32 [H, W], the input regions 1..N                      reached within `max_rounds` rounds
        out["root"]       numpy int32 [N + 1]: the surviving region id per input region (root[0] = 0)
        out["changed"]    uint8 [H, W], 1 where the class changed; only with return_changed=True

    `min_area`: an int (every class), a {class: int} dict (missing classes 0) or a sequence indexed by class; 0 means regions
    of that class are never absorbed. Regions are the connected components over all classes, class 0 included, with
    `connectivity` 4 or 8; pixels of `void_value` (None: there is none, and class 255 cannot be used) belong to no region
    and are copied through; adjacency is always 4-adjacency. The rule is the module's docstring. Pieces of equal output class
    that end up adjacent are NOT joined during the sieve: they keep competing as separate pieces, and the caller relabels the
    cleaned map (`label_regions`) to get them as one region. More than `max_regions` input regions or `max_pairs` adjacent
    pairs raise InsarError. 13 launches plus 3 per round on the current stream; the host reads the control words once per 4
    rounds and once, with the roots, at the end. `scratch`: a SieveScratch of this key to reuse (else allocated)."""
    who = "sieve_regions"
    H, W, T, void, (max_regions, max_pairs, max_rounds) = _check_args(mask, min_area, connectivity, void_value, max_regions, max_pairs,
                                                                      max_rounds, return_changed, scratch)
    dev = mask.device
    if scratch is None:
        scratch = SieveScratch(H, W, dev, max_regions, max_pairs, max_rounds)
    if scratch.regions is None:
        scratch.regions = RegionScratch(H, W, dev, max_regions)
        scratch.state_host = pinned(scratch.state.numel())
    out = torch.empty(H, W, dtype=torch.uint8, device=dev)
    labels = torch.empty(H, W, dtype=torch.int32, device=dev)
    changed = torch.empty(H, W, dtype=torch.uint8, device=dev) if return_changed else None
    table = scratch.regions.table
    with torch.cuda.device(dev):
        s = _lib.stream_ptr()
        scratch.thresholds.copy_(torch.from_numpy(T), non_blocking=False)
        args = (max_regions, max_pairs, max_rounds, ptr(scratch.scratch))
        call("insar_sieve_remap", ptr(mask), H, W, void, *args, s)
        # the labelling of regions.py over the remapped map: every class is foreground; `out` takes its cleaned-mask output
        _label_launch(scratch.remap, None, int(connectivity), 1, 0.0, max_regions, scratch.regions.scratch, table, labels, out)
        call("insar_sieve_pairs", ptr(labels), H, W, max_regions, *args, s)

        def first_read(ctrl):
            if ctrl[3]:
                raise InsarError(f"{who}: {int(ctrl[3])} pixels of class 255 with void_value=None: 255 classes at most")
            if ctrl[2] > max_regions:
                raise InsarError(f"{who}: {int(ctrl[2])} regions exceed max_regions={max_regions}: raise max_regions")
            if ctrl[1] or ctrl[0] > max_pairs:
                raise InsarError(f"{who}: {'more than ' if ctrl[1] else ''}{int(ctrl[0])} adjacent region pairs exceed "
                                 f"max_pairs={max_pairs}: raise max_pairs")

        rounds, converged, ctrl = merge_rounds(
            lambda first, n: call("insar_sieve_rounds", ptr(table), ptr(mask), ptr(scratch.thresholds), H, W, first, n, *args, s),
            scratch.ctrl_host, scratch.ctrl, max_rounds, first_read)
        N = int(ctrl[2])
        call("insar_sieve_apply", ptr(labels), ptr(mask), H, W, *args, ptr(out), ptr(changed), s)
        nbytes = scratch.ctrl.numel() + 4 * (N + 1)
        raw = read_back(scratch.state_host, scratch.state, nbytes)
    ctrl = raw[:scratch.ctrl.numel()].view(np.int32)
    res = {"mask": out, "regions_in": N, "absorbed": int(ctrl[5]), "changed_pixels": int(ctrl[4]), "rounds": rounds,
           "converged": converged, "labels_in": labels, "root": raw[scratch.ctrl.numel():nbytes].view(np.int32).copy()}
    if return_changed:
        res["changed"] = changed
    return res


__all__ = ["DEFAULT_MAX_PAIRS", "PAIR_DTYPE", "SieveScratch", "region_adjacency", "scratch_bytes", "sieve_regions", "threshold_table"]
