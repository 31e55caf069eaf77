"""What the scene tools (regions, score, distance, outlines, simplify, skeletons, zonal, split, rasterise, stack, warp, crops,
contours, focal, reconstruct) share on the host: the byte queries, the argument checks, the scratch buffers and the read-back. The host counterpart
of csrc/scene_common.h. Every refusal is an InsarError that names the tool (`who`) and the argument."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr


def query_bytes(name: str, *args, outputs: int):
    """The `outputs` int64 byte counts that the entry point `name` writes behind its integer arguments: one int, or a tuple.
    Host arithmetic only."""
    cells = [C.c_int64(0) for _ in range(outputs)]
    call(name, *map(int, args), *map(C.byref, cells))
    return int(cells[0].value) if outputs == 1 else tuple(int(c.value) for c in cells)


def is_int(v, *, integral_floats: bool = False) -> bool:
    """The two rules for an integer argument. The strict one takes int and np.integer alone; with `integral_floats` a finite
    float with an integral value passes too (3.0, never 1.5). Neither takes a bool."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating) if integral_floats else (int, np.integer)):
        return False
    return not isinstance(v, (float, np.floating)) or (math.isfinite(v) and int(v) == v)


def check_int(who: Optional[str], name: str, v, lo: int, hi: Optional[int] = None, *, integral_floats: bool,
              expect: Optional[str] = None) -> int:
    """int(v) of an integer (`is_int`) in lo..hi (hi=None: unbounded), else InsarError. `expect` words what was expected
    where the range alone reads badly."""
    if type(v) is int and v >= lo and (hi is None or v <= hi):              # the usual case, kept off the slow path
        return v
    if not is_int(v, integral_floats=integral_floats) or v < lo or (hi is not None and v > hi):
        expect = expect or (f"an integer in {lo}..{hi}" if hi is not None else f"an integer >= {lo}")
        raise InsarError(f"{who + ': ' if who else ''}{name}={v!r}: {expect}")
    return int(v)


def _names(dtypes) -> str:
    return " or ".join(str(d).replace("torch.", "") for d in dtypes)


_RANKS = {1: "1-D", 2: "2-D [H, W]", 3: "3-D [B, H, W]", 4: "4-D"}


def check_map(who: str, name: str, m, dtypes, *, dims=(2,), shape=None, of: str = "labels", one_fault: bool = False) -> None:
    """Refuse `m` unless it is a contiguous tensor of one of `dtypes` whose rank is in `dims` and whose last two dimensions
    are `shape`, those of the map named `of` (where given). Everything but the device, which is `check_on_device`'s: the
    tools differ in whether they look at it first or last. `one_fault` names the one property that failed (dtype, then rank,
    then contiguity) instead of all that is expected."""
    if not isinstance(m, torch.Tensor):
        raise InsarError(f"{who}: {name} must be a torch tensor, got {type(m).__name__}")
    if m.dtype not in dtypes or m.dim() not in dims or not m.is_contiguous():
        rank = "2-D" if tuple(dims) == (2,) else " or ".join(_RANKS[d] for d in dims)
        what = f"a contiguous {rank} {_names(dtypes)} tensor"
        if one_fault:
            what = _names(dtypes) if m.dtype not in dtypes else rank if m.dim() not in dims else "contiguous"
        raise InsarError(f"{who}: {name} must be {what}, got {m.dtype} {m.dim()}-D {tuple(m.shape)}")
    if shape is not None and tuple(m.shape[-2:]) != tuple(shape):
        raise InsarError(f"{who}: {name} {tuple(m.shape)}: expected {tuple(shape)} for {of}")


def check_on_device(who: str, name: str, m, like: Optional[torch.Tensor] = None) -> None:
    """Refuse `m` unless it is a tensor on a ROCm device: that of `like`, where given."""
    if not isinstance(m, torch.Tensor):
        raise InsarError(f"{who}: {name} must be a torch tensor on a ROCm device, got {type(m).__name__}")
    if not m.is_cuda or (like is not None and m.device != like.device):
        where = "" if like is None else f" on {like.device}, not {m.device}"
        raise InsarError(f"{who}: {name} must be a ROCm tensor{where} (no CPU fallback)")


def inverse_affine(transform):
    """(inverse of the 2 x 2 part, translation) of a 2 x 3 affine world = A @ (x, y, 1), in float64."""
    A = np.asarray(transform, dtype=np.float64)
    if A.shape != (2, 3):
        raise InsarError(f"transform must be a 2 x 3 affine, got shape {A.shape}")
    det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    if not np.isfinite(A).all() or det == 0:
        raise InsarError("transform is singular or not finite")
    inv = np.array([[A[1, 1], -A[0, 1]], [-A[1, 0], A[0, 0]]]) / det
    return inv, A[:, 2].copy()


def pinned(n: int, dtype: torch.dtype = torch.uint8) -> torch.Tensor:
    """A page-locked host buffer for a non-blocking read-back."""
    return torch.empty(n, dtype=dtype, pin_memory=True)


def read_back(host: torch.Tensor, dev: torch.Tensor, nbytes: Optional[int] = None) -> np.ndarray:
    """The first `nbytes` elements of `dev` (None: all) as the numpy view of `host`, after ONE non-blocking copy on the
    current stream and ONE synchronisation of it. Call it inside the caller's `torch.cuda.device(...)` block."""
    if nbytes is not None:
        host, dev = host[:nbytes], dev[:nbytes]
    host.copy_(dev, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy()


# ---- what simplify.py and contours.py share of Douglas-Peucker (csrc/dp_common.h) ------------------------------------------------
# A round is one level of the recursion: a record of n vertices that splits evenly is done after log2 n rounds (17 for 10^5
# vertices), one that sheds a vertex per level, like a spiral arm, needs as many rounds as vertices; 64 covers outlines and
# contour lines as detection produces them, and `converged` says when it did not.
DEFAULT_MAX_ROUNDS = 64
MAX_ROUNDS = 4095
ROUNDS_PER_READ = 8                      # the host looks at a round's counter once per this many rounds
MAX_TOLERANCE = 1024.0


def check_tolerance(who: str, name: str, tolerance) -> float:
    """The tolerance of a simplification in pixels: a finite number in 0 .. 1024, else InsarError."""
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.integer, np.floating)):
        raise InsarError(f"{who}: {name}={tolerance!r}: a number of pixels")
    if not math.isfinite(float(tolerance)) or not 0.0 <= float(tolerance) <= MAX_TOLERANCE:
        raise InsarError(f"{who}: {name}={tolerance!r}: finite, 0 .. {MAX_TOLERANCE:g}")
    return float(tolerance)


def simplify_rounds(prefix: str, scratch, v: torch.Tensor, n_records: int, nbytes: int, eps: int, max_rounds: int, setup_extra=()):
    """One simplification through the entry points `prefix`_setup / _rounds / _finish on the current stream of v's device: the
    first `nbytes` of the pinned input table `scratch.host_in` (filled by the caller: header + n_records records) go up, setup
    runs (`setup_extra` between the record count and the capacities), then batches of ROUNDS_PER_READ rounds until the 4-byte
    counter of a batch's last round reads 0 or the probe after `max_rounds` has run, then finish. Returns (the raw bytes of
    the output table, header first, a view of `scratch.host`; the compacted vertices; their input positions), the last two
    device tensors of full length of which the header's count says how much is used."""
    V = int(v.shape[0])
    out_v = torch.empty(V, 2, dtype=torch.int32, device=v.device)
    out_k = torch.empty(V, dtype=torch.int32, device=v.device)
    head = (ptr(v), V, ptr(scratch.table_in), n_records)
    caps = (*scratch.key()[:2], ptr(scratch.scratch))            # max_vertices, max records, scratch
    with torch.cuda.device(v.device):
        s = _lib.stream_ptr()
        scratch.table_in[:nbytes].copy_(scratch.host_in[:nbytes], non_blocking=True)
        call(prefix + "_setup", *head, *setup_extra, *caps, s)
        r, total = 0, max_rounds + 1                             # the last round is the probe
        while r < total:
            n = min(ROUNDS_PER_READ, total - r)
            call(prefix + "_rounds", *head, eps, r, n, max_rounds, *caps, s)
            r += n
            if r < total and int(read_back(scratch.counter, scratch.scratch[4 * (r - 1):4 * r]).view(np.int32)[0]) == 0:
                break
        call(prefix + "_finish", *head, max_rounds, *caps, ptr(scratch.table), ptr(out_v), ptr(out_k), s)
        return read_back(scratch.host, scratch.table, nbytes), out_v, out_k


# ---- what sieve.py and split.py share: pieces that merge in synchronous rounds until a round merges nothing ----------------------
MERGE_ROUNDS_PER_READ = 4                # the host looks at the rounds' counters once per this many rounds
# int32 control words of the tool's own, then one merge counter per round: SV_CTRL_WORDS of csrc/sieve.hip and SP_CTRL_WORDS of
# csrc/split.hip, which lay their words out separately, must both equal it
MERGE_CTRL_WORDS = 8


def merge_rounds(run, ctrl_host: torch.Tensor, ctrl: torch.Tensor, max_rounds: int, first_read):
    """Batches of MERGE_ROUNDS_PER_READ rounds, `run(first_round, n_rounds)` launching a batch, with ONE read-back of the
    control words `ctrl` (into the pinned `ctrl_host`) behind each, until a round's counter reads 0 or `max_rounds` rounds
    have run. `first_read(words)` sees the first read-back: the tool's capacity checks. Returns (rounds that merged
    something, whether an idle round was reached, the int32 control words as last read). Call it inside the caller's
    `torch.cuda.device(...)` block."""
    done, rounds, converged = 0, max_rounds, False
    while done < max_rounds and not converged:
        n = min(MERGE_ROUNDS_PER_READ, max_rounds - done)
        run(done, n)
        words = read_back(ctrl_host, ctrl).view(np.int32)
        if done == 0:
            first_read(words)
        done += n
        idle = np.flatnonzero(words[MERGE_CTRL_WORDS:MERGE_CTRL_WORDS + done] == 0)
        if len(idle):                                             # rounds after the first idle one changed nothing
            rounds, converged = int(idle[0]), True
    return rounds, converged, words


class Scratch:
    """The buffers of one tool for one key (a scene size, capacities) on one device. A subclass names its key in KEY (the
    names become attributes), says where `device` stands among its constructor's arguments, and hands its byte counts to
    `__init__`. Nothing in the buffers has to survive between calls."""
    KEY: tuple = ()
    SHOW: Optional[str] = None           # how a key reads in a refusal; None: name=value, ...
    DEVICE_AT = 0                        # the constructor is cls(*key) with `device` inserted here

    def __init__(self, key, device, *, host: Optional[int] = None, **nbytes):
        """uint8 device tensors named by `nbytes`, of that many bytes each (a tensor is taken as it is), and a pinned `host` of
        `host` bytes."""
        for n, v in zip(self.KEY, key):
            setattr(self, n, int(v))
        for n, b in nbytes.items():
            setattr(self, n, b if isinstance(b, torch.Tensor) else torch.empty(b, dtype=torch.uint8, device=device))
        if host is not None:
            self.host = pinned(host)

    def key(self) -> tuple:
        return tuple(getattr(self, n) for n in self.KEY)

    @property
    def device(self) -> torch.device:
        return _device_of(self)

    @staticmethod
    def adopt_table(who: str, table, nbytes: int):
        """What `__init__` takes as the table's size: `nbytes` (a fresh allocation) without a caller's `table`, else that
        tensor, refused unless it holds exactly `nbytes` bytes in a layout the kernels can take."""
        if table is None:
            return nbytes
        if (not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or table.dim() != 1 or table.numel() != nbytes
                or not table.is_contiguous() or table.data_ptr() % 16):
            raise InsarError(f"{who}: table must be a contiguous 16-byte aligned uint8 tensor of {nbytes} bytes")
        return table

    @classmethod
    def show(cls, key) -> str:
        return cls.SHOW.format(*key) if cls.SHOW else ", ".join(f"{n}={v}" for n, v in zip(cls.KEY, key))

    @classmethod
    def check(cls, who: str, scratch, key, device=None, *, table_bytes: Optional[int] = None) -> None:
        """Refuse a caller's `scratch` that is not one of `key` on `device` (None: not looked at) or, with `table_bytes`,
        whose table is not of that size. Where the table's size is verified, anything that carries the key's attributes and
        such a table will do."""
        if not (isinstance(scratch, cls) or (table_bytes is not None and all(hasattr(scratch, n) for n in cls.KEY))):
            raise InsarError(f"{who}: scratch must be a {cls.__name__}, got {type(scratch).__name__}")
        got, table = tuple(getattr(scratch, n) for n in cls.KEY), getattr(scratch, "table", None)
        sized = table_bytes is None or (isinstance(table, torch.Tensor) and table.numel() == table_bytes)
        if got != tuple(key) or not sized or (device is not None and _device_of(scratch) != device):
            raise InsarError(f"{who}: scratch of {cls.show(got)} on {_device_of(scratch)} for {cls.show(key)} on {device}"
                             + ("" if sized else f" ({table_bytes} bytes)"))

    @classmethod
    def build(cls, device, *key):
        """A scratch of `key` on `device`, or None if the key is not made of plain integers that the tool's byte query takes:
        the tool itself then refuses the argument by name."""
        if not all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in key):
            return None
        args = list(key)
        args.insert(cls.DEVICE_AT, device)
        try:
            return cls(*args)
        except InsarError:
            return None


def _device_of(scratch):
    for n in ("scratch", "table"):
        if isinstance(getattr(scratch, n, None), torch.Tensor):
            return getattr(scratch, n).device
    return None
