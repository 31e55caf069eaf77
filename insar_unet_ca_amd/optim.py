"""optim.Adam(lr=1e-4) of the reference's training loop (Unet-ChannalAttention.py:466,346)
as one multi-tensor HIP launch. State (`step`, `exp_avg`, `exp_avg_sq`) is kept in
torch.optim.Adam's own format, so optimizer.state_dict() interchanges with the reference's."""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import struct

import torch

from . import _lib
from ._lib import call, ptr

# elements per work-group of the Adam launch (256 threads): small enough for every CU to hold several work-groups for the
# whole launch. 31 M parameters in one buffer, stand-alone (tools/pass_bench.py): 64 Ki 177 us, 16 Ki 175, 8 Ki 166, 4 Ki 165.
CHUNK = int(os.environ.get("INSAR_ADAM_CHUNK", "8192"))


# ---- what Adam, AdamW and parallel.ShardedAdam share: launch tables, their cache, the in-place state restore ---------------
def build_tables(rows, numels, dev):
    """The two device tensors every Adam-family kernel reads: `rows` (one list of integer words per tensor, equal widths:
    pointers, element count, float bits) as the int64 table [n, width], and one [tensor, chunk] int32 pair per CHUNK elements
    of each tensor (`numels`, in row order). Returns (table, chunk_t, nchunks)."""
    chunks = [[ti, ci] for ti, n in enumerate(numels) for ci in range((n + CHUNK - 1) // CHUNK)]
    return torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(chunks, dtype=torch.int32).to(dev), len(chunks)


def rows_key(rows) -> tuple:
    """Cache key of a table: every word of every row, so a gradient or moment tensor that moved never replays an old table."""
    return tuple(map(tuple, rows))


class TableCache(dict):
    """key -> launch entry ((table, chunk_t, nchunks, ...)). Bounded: emptied when it holds more than 8 entries."""

    def put(self, key, entry):
        if len(self) > 8:
            self.clear()
        self[key] = entry
        return entry


def adam_tables(cache: TableCache, tensors, key=None):
    """(table, chunk_t, nchunks) of the plain Adam kernel for (p, g, m, v) tuples: 5 words per row."""
    rows = [[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()] for p, g, m, v in tensors]
    key = rows_key(rows) if key is None else key
    hit = cache.get(key)
    if hit is None:
        hit = cache.put(key, build_tables(rows, [r[4] for r in rows], tensors[0][0].device))
    return hit


def restore_in_place(old, state) -> bool:
    """After torch's load_state_dict has built fresh state tensors in `state`: copy them into the tensors `old` (parameter ->
    its state before the load) held wherever shape, dtype and device agree, and put those back, so that their addresses
    stay what pointer tables and a captured hipGraph hold. True if nothing had to be re-allocated and no parameter lost
    its state."""
    in_place = True
    for p, st in state.items():
        prev = old.get(p)
        for k in ("exp_avg", "exp_avg_sq", "step"):
            new, keep = st.get(k), (prev.get(k) if prev else None)
            if (torch.is_tensor(new) and torch.is_tensor(keep) and keep.shape == new.shape and keep.dtype == new.dtype
                    and keep.device == new.device):
                keep.copy_(new)
                st[k] = keep
            elif new is not None:
                in_place = False
    return in_place and not set(old) - set(state)


def _require_device(p, g, who="AdamW", one_text=False) -> None:
    typed = p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous()
    if one_text and not (p.is_cuda and typed):       # Adam on the device-side step count words both refusals as one
        raise _lib.InsarError(f"{who} HIP path: contiguous float32 ROCm parameters and gradients only")
    if not p.is_cuda:
        raise _lib.InsarError(f"{who} HIP path: parameters must live on a ROCm device (no CPU fallback)")
    if not typed:
        raise _lib.InsarError(f"{who} HIP path: contiguous float32 parameters and gradients only")


class Adam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kw):
        if weight_decay != 0 or amsgrad or kw.get("maximize") or kw.get("capturable") or kw.get("differentiable"):
            raise _lib.InsarError("Adam HIP path: weight_decay=0, amsgrad=False, maximize=False only")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, foreach=False, fused=False)
        self._tables = TableCache()
        self.grad_scale = 1.0      # multiplies every gradient inside the kernel (DP pre-scaling)
        self._dev_state = None     # float[4] on the device: step count + bias corrections (enable_device_step)
        self._dev_pending = 0      # steps taken on the device that state['step'] has not been told about yet
        self._fast = None          # (params, grads, step tensors, table, chunks, nchunks, param addresses) of the last full step
        self.generation = 0        # bumped whenever optimizer state had to be re-allocated (see load_state_dict)
        self._early_tables = {}    # (plan id, stage, gradient buffer) -> (table, chunks, nchunks, params)
        self._early_done = set()   # ids of the parameters already updated inside the current backward
        self._early_stages = 0

    # ---- device-side step count (hipGraph capture) ---------------------------------------------------------
    def enable_device_step(self) -> None:
        """Keep the step count and the bias corrections in device memory (insar_adam_step_dev): the launch arguments of
        `step()` then never change, which is what a captured hipGraph of the training step needs. The arithmetic is the
        same (bias corrections computed in double, rounded to fp32: bitwise the eager path's parameters). Requires every
        parameter to share one step count; `state_dict()` still reports torch.optim.Adam's per-parameter `step`."""
        if self._dev_state is not None:
            return
        steps, dev = set(), None
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p, {})
                steps.add(float(st["step"]) if "step" in st else 0.0)
                dev = p.device
        if len(steps) > 1:
            raise _lib.InsarError("Adam.enable_device_step: parameters have different step counts")
        if len({tuple(g["betas"]) for g in self.param_groups}) > 1:
            raise _lib.InsarError("Adam.enable_device_step: one (beta1, beta2) for all parameter groups")
        t = steps.pop() if steps else 0.0
        b1, b2 = self.param_groups[0]["betas"]
        self._dev_state = torch.tensor([t, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), 0.0], dtype=torch.float32).to(dev)

    # ---- optimizer inside backward ------------------------------------------------------------------------
    def fuse_into_backward(self, model) -> "Adam":
        """Run this optimizer STAGE BY STAGE inside `loss.backward()`: as soon as a backward stage of `model` (a decoder /
        encoder block: engine.grad_groups) has enqueued its last gradient kernel, Adam updates that stage's parameters on the
        weight-gradient side stream and the stage's GEMM-layout weight copies are rebuilt right behind it — beside the rest of
        backward instead of after it (the reference's loop runs optimizer.step() after loss.backward(), :345-346; same
        arithmetic, same order per parameter, so the parameters are bit for bit those of the plain step). `step()` then only
        finishes what is left (nothing, in the steady state) and advances the step counts.
        MEASURED SLOWER on config 2 (same-box A/B 7.77 -> 8.29 ms/step, profiles/r03_adam_in_backward_ab.txt: 875 MB of optimizer
        traffic and 18 extra launches beside the dgrad chain cost more than the 0.17 ms of exposed Adam they hide), so nothing
        in this repository turns it on; it stays as a tested option for steps with a different balance.
        Contract of the opt-in: ONE backward per step() (no gradient accumulation over several backward calls: a second
        backward before step() raises), nobody reads the parameters between backward and step(), one parameter group, no
        data-parallel wrapper (there the gradients are final only after the exchange; the plain step is used)."""
        hooks = getattr(model, "_hooks", None)
        if hooks is None:
            raise _lib.InsarError("Adam.fuse_into_backward: the model has no HIP plan hooks (UNet / DeepLabV3_SingleChannel_Attn)")
        hooks["on_stage_optim"] = self._early_stage
        return self

    def _early_stage(self, plan, stage: int) -> None:
        if stage < 0:                            # backward begins
            if self._early_done:
                raise _lib.InsarError("Adam.fuse_into_backward: a second backward before optimizer.step() — the first one has "
                                      "already updated parameters; gradient accumulation needs the plain step")
            self._early_stages = 0
            return
        f = self._fast
        if (f is None or self._dev_state is not None or len(self.param_groups) != 1 or torch.cuda.is_current_stream_capturing()
                or stage >= len(plan.sink.groups)):
            return                               # not in the steady state yet (first steps build the optimizer state): plain step()
        from . import engine
        group = self.param_groups[0]
        key = (id(plan), stage, plan.sink.active)
        hit = self._early_tables.get(key)
        if hit is None:
            params = plan.sink.groups[stage]
            tensors = []
            for p in params:
                st = self.state.get(p)
                if not p.requires_grad or st is None or "exp_avg" not in st:
                    return
                tensors.append((p, plan.sink.view(p), st["exp_avg"], st["exp_avg_sq"]))
            if not tensors:
                return
            if len(self._early_tables) > 64:
                self._early_tables.clear()
            hit = self._early_tables[key] = adam_tables(self._tables, tensors, ("early",) + key) + ([t[0] for t in tensors],)
        table, chunk_t, nchunks, params = hit
        with plan.ctx.side_stream():             # ordered after everything this stage has enqueued on either stream
            self._launch(group, table, chunk_t, nchunks, float(self.state[params[0]]["step"]) + 1.0)
            torch._C._increment_version(params)
            ws = plan.weightset.stage_sets(plan.sink.groups)[stage]
            if ws is not None and engine.PREP_SIDE:
                ws.refresh()                     # this stage's GEMM-layout copies: the next forward finds them current
        self._early_done.update(id(p) for p in params)
        self._early_stages += 1

    def _finish_early(self) -> bool:
        """step() after a backward that ran (some of) the update itself. True if nothing is left to do."""
        done, self._early_done = self._early_done, set()
        group = self.param_groups[0]
        rest = [p for p in group["params"] if p.grad is not None and id(p) not in done]
        t = float(self.state[group["params"][0]]["step"]) + 1.0
        if rest:                                 # stages that did not take part (a plan change mid-way): the same kernel on them
            tensors = [(p, p.grad, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in rest]
            self._launch(group, *adam_tables(self._tables, tensors), t)
            torch._C._increment_version(rest)
        for p in group["params"]:
            st = self.state.get(p)
            if st is not None and "step" in st and (p.grad is not None or id(p) in done):
                st["step"] += 1
        return True

    def _sync_host_steps(self) -> None:
        if self._dev_pending:
            for group in self.param_groups:
                for p in group["params"]:
                    st = self.state.get(p)
                    if st is not None and "step" in st:
                        st["step"] += self._dev_pending
            self._dev_pending = 0

    def state_dict(self):
        self._sync_host_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Restores IN PLACE wherever the optimizer already holds state of the same shape: the moment tensors, the step
        counters and the device-side step state keep their addresses, so cached pointer tables and a captured hipGraph
        (graph.GraphedTrainStep bakes those addresses into its kernel nodes) stay valid and see the restored values.
        State that has to be re-allocated (first load, changed shapes) bumps `generation`, which GraphedTrainStep checks."""
        self._sync_host_steps()
        old = {p: dict(st) for p, st in self.state.items()}
        super().load_state_dict(state_dict)          # builds fresh state tensors
        if not restore_in_place(old, self.state):
            self._fast = None
            self._tables.clear()
            self._early_tables.clear()
            self.generation += 1
        if self._dev_state is not None:
            self._dev_pending = 0
            keep, self._dev_state = self._dev_state, None
            self.enable_device_step()                # validates the loaded step counts, builds the new values
            keep.copy_(self._dev_state)              # ... which go into the tensor a captured graph already points at
            self._dev_state = keep

    def _launch(self, group, table, chunk_t, nchunks, t=None) -> None:
        """The one launch site of both kernels. t: the step count this update is, held by the host (the bias corrections
        are computed here, in double); None: the count lives on the device (enable_device_step)."""
        b1, b2 = group["betas"]
        head = (ptr(table), ptr(chunk_t), nchunks, CHUNK, float(group["lr"]), float(b1), float(b2), float(group["eps"]))
        if t is None:
            call("insar_adam_step_dev", *head, ptr(self._dev_state), float(self.grad_scale), _lib.stream_ptr())
        else:
            call("insar_adam_step", *head, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), float(self.grad_scale), _lib.stream_ptr())

    def _fast_step(self) -> bool:
        """The steady-state step: same parameters, same gradient tensors (the flat-buffer views the model hands out every
        step) and optimizer state as the last full step -> reuse its pointer table; the per-parameter bookkeeping of
        torch.optim.Adam (_init_group, 400 data_ptr calls) costs 0.7-1.2 ms of host time per step otherwise."""
        f = self._fast
        if f is None or len(self.param_groups) != 1:
            return False
        params, grads, steps, table, chunk_t, nchunks, ptrs = f
        group = self.param_groups[0]
        if len(group["params"]) != len(params):
            return False
        for p, q, g, a in zip(group["params"], params, grads, ptrs):
            # same Parameter, same gradient tensor AND the same parameter storage: `p.data = ...` / load_state_dict(assign=True)
            # keep the Parameter object but move its memory, and the table holds raw addresses
            if p is not q or p.grad is not g or p.data_ptr() != a:
                return False
        if self._dev_state is not None:
            self._launch(group, table, chunk_t, nchunks)
        else:
            for st in steps:
                st += 1
            self._launch(group, table, chunk_t, nchunks, float(steps[0]))
        torch._C._increment_version(params)
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if closure is None and self._early_done:
            self._finish_early()
            return loss
        if closure is None and self._fast_step():
            if self._dev_state is not None:
                self._dev_pending += 1
            return loss
        self._fast = None
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps = [], [], [], [], [], []
            self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps)
            if not params:
                continue
            on_dev = self._dev_state is not None
            by_step = {}                             # step count -> its tensors, one launch each (None: the device counts)
            for p, g, m, v, st in zip(params, grads, exp_avgs, exp_avg_sqs, steps):
                _require_device(p, g, "Adam", one_text=on_dev)
                if not on_dev:
                    st += 1
                by_step.setdefault(None if on_dev else float(st), []).append((p, g, m, v))
            for t, tensors in by_step.items():
                table, chunk_t, nchunks = adam_tables(self._tables, tensors)
                self._launch(group, table, chunk_t, nchunks, t)
                torch._C._increment_version([p for p, _, _, _ in tensors])
            if len(self.param_groups) == 1 and len(by_step) == 1 and len(params) == len(group["params"]):
                self._fast = (list(params), list(grads), list(steps), table, chunk_t, nchunks, [p.data_ptr() for p in params])
        if self._dev_state is not None:
            self._dev_pending += 1
        return loss


# ---- AdamW: decoupled decay, global-norm clip, learning-rate schedule and EMA weights, all on the device ------------------
class LRSchedule:
    """Settings of the learning-rate schedule AdamW evaluates ON THE DEVICE (csrc/optim_w.hip: optw_lr), per step, not per
    epoch: linear warm-up from `warmup_start * lr` over `warmup_steps` steps, then `constant`, `cosine` or `poly` (exponent
    `power`; DeepLab's recipe is poly 0.9) down to `min_lr` at `total_steps`, held there afterwards."""
    KINDS = {"constant": _lib.SCHED_CONSTANT, "cosine": _lib.SCHED_COSINE, "poly": _lib.SCHED_POLY}

    def __init__(self, kind: str, total_steps=None, warmup_steps: int = 0, warmup_start: float = 0.0, min_lr: float = 0.0,
                 power: float = 0.9):
        if kind not in self.KINDS:
            raise _lib.InsarError(f"LRSchedule: kind {kind!r} (constant | cosine | poly)")
        if warmup_steps < 0 or not 0.0 <= warmup_start <= 1.0 or min_lr < 0 or power <= 0:
            raise _lib.InsarError("LRSchedule: warmup_steps >= 0, 0 <= warmup_start <= 1, min_lr >= 0, power > 0")
        if kind != "constant" and (total_steps is None or int(total_steps) <= warmup_steps):
            raise _lib.InsarError(f"LRSchedule: {kind} needs total_steps > warmup_steps")
        self.kind, self.total_steps = kind, (0 if total_steps is None else int(total_steps))
        self.warmup_steps, self.warmup_start, self.min_lr, self.power = int(warmup_steps), float(warmup_start), float(min_lr), float(power)

    def lr_at(self, base_lr: float, t: int) -> float:
        """The learning rate of the step taken after `t` finished steps (t = 0: the first step), in Python floats: the
        host restatement of the kernel's formula (LambdaLR's convention: its factor at epoch t)."""
        if t < self.warmup_steps:
            return base_lr * (self.warmup_start + (1.0 - self.warmup_start) * (t / self.warmup_steps))
        if self.kind == "constant":
            return base_lr
        if t >= self.total_steps:
            return self.min_lr
        q = (t - self.warmup_steps) / (self.total_steps - self.warmup_steps)
        if self.kind == "cosine":
            return self.min_lr + (base_lr - self.min_lr) * (0.5 * (1.0 + math.cos(math.pi * q)))
        return self.min_lr + (base_lr - self.min_lr) * (1.0 - q) ** self.power


def split_decay_groups(model, weight_decay: float):
    """Two parameter groups for AdamW: biases, BatchNorm affine parameters and every other parameter with ndim <= 1 are
    exempt from weight decay; the rest get `weight_decay`."""
    decay = [p for p in model.parameters() if p.requires_grad and p.ndim > 1]
    exempt = [p for p in model.parameters() if p.requires_grad and p.ndim <= 1]
    return [{"params": decay, "weight_decay": float(weight_decay)}, {"params": exempt, "weight_decay": 0.0}]


def _float_bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


class AdamW(torch.optim.AdamW):
    """torch.optim.AdamW's update as at most three HIP launches per step (include/insar_hip.h: insar_gradnorm_partials ->
    insar_optw_advance -> insar_adamw_step), with what a segmentation recipe adds around it done on the device:
    `max_grad_norm` (clip_grad_norm_'s global-norm clip, no host sync), `schedule` (an LRSchedule, evaluated per step),
    `ema_decay` (an exponential moving average of the weights, updated in the same pass), `skip_nonfinite` (a step whose
    gradient norm is inf / NaN changes nothing and is counted). Step count, bias corrections, learning rate, clip
    coefficient and EMA factor live in one device-side state block, so the launch arguments never change and
    GraphedTrainStep can capture the step. `decoupled=False` gives Adam's L2 form (g += wd * p) instead.
    Parameter groups may differ in `weight_decay` and `lr` (group lr / first group's lr scales the scheduled rate); betas
    and eps are common. `param_groups[i]["lr"]` keeps the base value; `get_last_lr()` is the scheduled one.
    state_dict() is torch.optim.AdamW's (per-parameter step / exp_avg / exp_avg_sq) plus one top-level entry
    "insar_adamw" = {"skipped": int, "ema": {parameter index: tensor}}, which torch's load_state_dict ignores."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, decoupled=True, max_grad_norm=None,
                 skip_nonfinite=False, schedule=None, ema_decay=None, ema_warmup=True):
        if max_grad_norm is not None and not max_grad_norm >= 0:
            raise _lib.InsarError(f"AdamW: max_grad_norm={max_grad_norm} must be >= 0 (None: no clipping)")
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise _lib.InsarError(f"AdamW: ema_decay={ema_decay} outside [0, 1)")
        if schedule is not None and not isinstance(schedule, LRSchedule):
            raise _lib.InsarError("AdamW: schedule is an LRSchedule (or None)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False, fused=False)
        if len({(tuple(g["betas"]), g["eps"]) for g in self.param_groups}) > 1:
            raise _lib.InsarError("AdamW: one (beta1, beta2) and one eps for all parameter groups")
        if any(g["lr"] <= 0 for g in self.param_groups):
            raise _lib.InsarError("AdamW: lr must be positive")
        self.decoupled, self.max_grad_norm, self.skip_nonfinite = bool(decoupled), max_grad_norm, bool(skip_nonfinite)
        self.schedule, self.ema_decay, self.ema_warmup = schedule, ema_decay, bool(ema_warmup)
        self.grad_scale = 1.0      # multiplies every gradient inside the kernels (DP pre-scaling); the norm sees it too
        self.generation = 0        # bumped whenever optimizer state had to be re-allocated (see load_state_dict)
        self._dev_state = None     # InsarOptwState in device memory (12 int32 words), made at the first step / load
        self._dev_pending = 0      # steps enqueued since the host last synced its step count
        self._host_t = 0           # step count as of the last sync
        self._ema = {}             # parameter -> its EMA tensor
        self._tables = TableCache()
        self._fast = None

    def enable_device_step(self) -> None:
        """The state is always on the device: nothing to do (GraphedTrainStep calls this)."""

    @property
    def _norm_pass(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    # ---- device-side state block ------------------------------------------------------------------------------
    def _state_block(self, dev) -> torch.Tensor:
        if self._dev_state is None:
            self._dev_state = torch.zeros(12, dtype=torch.int32, device=dev)
            self._write_state(self._host_t, 0)
        return self._dev_state

    def _write_state(self, t: int, skipped: int) -> None:
        """t, the skipped count and everything derived from t, as insar_optw_advance leaves them after step t."""
        b1, b2 = self.param_groups[0]["betas"]
        host = torch.zeros(12, dtype=torch.int32)
        host.view(torch.int64)[0:2] = torch.tensor([t, skipped], dtype=torch.int64)
        alpha = 0.0 if self.ema_decay is None else 1.0 - self._decay_at(t)
        host.view(torch.float32)[4:10] = torch.tensor([1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), self._lr_at(max(t - 1, 0)), 1.0,
                                                       0.0, alpha], dtype=torch.float64).float()
        self._dev_state.copy_(host)

    def _read_state(self):
        host = self._dev_state.cpu()                         # synchronises: logging / checkpoint paths only
        i64, f32 = host.view(torch.int64), host.view(torch.float32)
        return {"t": int(i64[0]), "skipped": int(i64[1]), "bc1": float(f32[4]), "bc2_sqrt": float(f32[5]), "lr": float(f32[6]),
                "coef": float(f32[7]), "grad_norm": float(f32[8]), "ema_alpha": float(f32[9]), "skip": int(host[10])}

    def _decay_at(self, t: int) -> float:
        return min(self.ema_decay, (1.0 + t) / (10.0 + t)) if self.ema_warmup else self.ema_decay

    def _lr_at(self, done: int) -> float:
        base = float(self.param_groups[0]["lr"])
        return base if self.schedule is None else self.schedule.lr_at(base, done)

    def _config(self) -> "_lib.InsarOptwConfig":
        b1, b2 = self.param_groups[0]["betas"]
        s = self.schedule
        return _lib.InsarOptwConfig(
            float(self.param_groups[0]["lr"]), float(b1), float(b2), -1.0 if self.max_grad_norm is None else float(self.max_grad_norm),
            s.warmup_start if s else 0.0, s.min_lr if s else 0.0, s.power if s else 1.0,
            -1.0 if self.ema_decay is None else float(self.ema_decay), s.warmup_steps if s else 0, s.total_steps if s else 0,
            LRSchedule.KINDS[s.kind] if s else _lib.SCHED_NONE, int(self.skip_nonfinite), int(self.ema_warmup), 0)

    # ---- read-backs (never on the step path) -----------------------------------------------------------------
    def _sync_host_steps(self) -> None:
        if self._dev_pending and self.skip_nonfinite and self._dev_state is not None:
            self._host_t = self._read_state()["t"]           # skipped steps do not count: only the device knows
        else:
            self._host_t += self._dev_pending
        self._dev_pending = 0
        for st in self.state.values():
            if "step" in st:
                st["step"].fill_(float(self._host_t))

    def get_last_lr(self):
        """The learning rate the last step used, per parameter group, from the host's step count and LRSchedule.lr_at:
        no device read-back (with skip_nonfinite the step count itself has to be read)."""
        self._sync_host_steps()
        lr = self._lr_at(max(self._host_t - 1, 0))
        base = float(self.param_groups[0]["lr"])
        return [lr * (float(g["lr"]) / base) for g in self.param_groups]

    def last_grad_norm(self) -> float:
        """Global gradient norm of the last step (after grad_scale, before clipping). Synchronises."""
        if not self._norm_pass or self._dev_state is None:
            raise _lib.InsarError("AdamW.last_grad_norm: needs max_grad_norm or skip_nonfinite, and one step taken")
        return self._read_state()["grad_norm"]

    def skipped_steps(self) -> int:
        """Steps skipped so far because their gradient norm was inf / NaN. Synchronises."""
        return 0 if self._dev_state is None else self._read_state()["skipped"]

    # ---- EMA weights -------------------------------------------------------------------------------------------
    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _swap_ema(self) -> None:
        if self.ema_decay is None or not self._ema:
            raise _lib.InsarError("AdamW.ema_weights: no EMA (ema_decay=None, or no step taken yet)")
        with torch.no_grad():
            for p, e in self._ema.items():
                tmp = p.detach().clone()
                p.copy_(e)                                   # in place: addresses stay, the version counter moves
                e.copy_(tmp)

    @contextlib.contextmanager
    def ema_weights(self):
        """with opt.ema_weights(): validate_model(...) / ScenePredictor(...) run on the averaged weights. EMA and live values
        are swapped in place on entry and swapped back on exit: addresses are kept (pointer tables and captured graphs stay
        valid) and the parameters' version counters move both times, so the engine re-lays its GEMM-layout weight copies.
        BatchNorm running statistics are buffers and are used as they are. No step() inside."""
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    def ema_state_dict(self, model):
        """`model.state_dict()` with every parameter this optimizer averages replaced by its EMA (clones): what to save as
        the .pth of the averaged model."""
        if self.ema_decay is None or not self._ema:
            raise _lib.InsarError("AdamW.ema_state_dict: no EMA (ema_decay=None, or no step taken yet)")
        names = {id(p): n for n, p in model.named_parameters()}
        sd = type(model.state_dict())((k, v.detach().clone()) for k, v in model.state_dict().items())
        for p, e in self._ema.items():
            if id(p) in names:
                sd[names[id(p)]] = e.detach().clone()
        return sd

    # ---- checkpoints ---------------------------------------------------------------------------------------------
    def state_dict(self):
        self._sync_host_steps()
        sd = super().state_dict()
        index = {id(p): i for i, p in enumerate(self._params())}
        sd["insar_adamw"] = {"skipped": self.skipped_steps(), "ema": {index[id(p)]: e for p, e in self._ema.items()}}
        return sd

    def load_state_dict(self, state_dict):
        """Restores IN PLACE wherever the optimizer already holds state of the same shape (moments, EMA, the device-side
        state block keep their addresses: pointer tables and a captured hipGraph stay valid); anything that has to be
        re-allocated bumps `generation`, which GraphedTrainStep checks — as Adam.load_state_dict."""
        self._sync_host_steps()
        extra = state_dict.get("insar_adamw") or {}
        old = {p: dict(st) for p, st in self.state.items()}
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "insar_adamw"})
        in_place = restore_in_place(old, self.state)
        steps = {float(st["step"]) for st in self.state.values() if "step" in st}
        if len(steps) > 1:
            raise _lib.InsarError("AdamW.load_state_dict: parameters have different step counts")
        params = self._params()
        old_ema, self._ema = self._ema, {}
        for i, e in (extra.get("ema") or {}).items():
            p = params[int(i)]
            keep = old_ema.get(p)
            if keep is not None and keep.shape == e.shape:
                keep.copy_(e)
            else:
                keep, in_place = e.detach().to(device=p.device, dtype=torch.float32).clone(), False
            self._ema[p] = keep
        if set(old_ema) - set(self._ema):
            in_place = False
        if not in_place:
            self._fast = None
            self._tables.clear()
            self.generation += 1
        self._host_t, self._dev_pending = int(steps.pop()) if steps else 0, 0
        if params:
            self._state_block(params[0].device)
            self._write_state(self._host_t, int(extra.get("skipped", 0)))

    # ---- the step --------------------------------------------------------------------------------------------------
    def _table(self, tensors):
        """(table, chunk_t, nchunks, partials, config) for (p, g, m, v, ema, weight decay, lr multiplier) tuples: 8 words per
        row, the two floats as their float32 bits; cached by the rows and the hyper-parameters the config is made from."""
        rows = [[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(e), p.numel(), _float_bits(wd), _float_bits(mult)]
                for p, g, m, v, e, wd, mult in tensors]
        key = (rows_key(rows), self._hyper())
        hit = self._tables.get(key)
        if hit is None:
            dev = tensors[0][0].device
            table, chunk_t, nchunks = build_tables(rows, [r[5] for r in rows], dev)
            partials = torch.zeros(nchunks, dtype=torch.float32, device=dev) if self._norm_pass else None
            hit = self._tables.put(key, (table, chunk_t, nchunks, partials, self._config()))
        return hit

    def _launch(self, table, chunk_t, nchunks, partials, cfg) -> None:
        b1, b2 = self.param_groups[0]["betas"]
        stream, state, gs = _lib.stream_ptr(), ptr(self._dev_state), float(self.grad_scale)
        if partials is not None:
            call("insar_gradnorm_partials", ptr(table), ptr(chunk_t), nchunks, CHUNK, gs, ptr(partials), stream)
        call("insar_optw_advance", ctypes.byref(cfg), ptr(partials), nchunks if partials is not None else 0, state, stream)
        call("insar_adamw_step", ptr(table), ptr(chunk_t), nchunks, CHUNK, float(b1), float(b2), float(self.param_groups[0]["eps"]),
             gs, int(self.decoupled), state, stream)

    def _hyper(self):
        return tuple((float(g["lr"]), float(g["weight_decay"]), tuple(g["betas"]), g["eps"]) for g in self.param_groups)

    def _fast_step(self) -> bool:
        """Steady state: the same parameters, gradient tensors, storage and hyper-parameters as the last full step -> the
        same pointer table (see Adam._fast_step)."""
        f = self._fast
        if f is None:
            return False
        params, grads, ptrs, hyper, launch = f
        if hyper != self._hyper():
            return False
        n = 0
        for group in self.param_groups:
            for p in group["params"]:
                if n >= len(params) or p is not params[n] or p.grad is not grads[n] or p.data_ptr() != ptrs[n]:
                    return False
                n += 1
        if n != len(params):
            return False
        self._launch(*launch)
        torch._C._increment_version(params)
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if closure is None and self._fast_step():
            self._dev_pending += 1
            return loss
        self._fast = None
        if len({(tuple(g["betas"]), g["eps"]) for g in self.param_groups}) > 1:
            raise _lib.InsarError("AdamW: one (beta1, beta2) and one eps for all parameter groups")
        base = float(self.param_groups[0]["lr"])
        tensors, every = [], True
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    every = False
                    continue
                _require_device(p, p.grad)
                st = self.state[p]
                if "exp_avg" not in st:
                    if self._host_t + self._dev_pending > 0:
                        raise _lib.InsarError("AdamW: a parameter got its first gradient after other parameters had already "
                                              "been stepped; every parameter shares one step count")
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                ema = None
                if self.ema_decay is not None:
                    ema = self._ema.get(p)
                    if ema is None:
                        ema = self._ema[p] = p.detach().clone(memory_format=torch.contiguous_format)
                tensors.append((p, p.grad, st["exp_avg"], st["exp_avg_sq"], ema, float(group["weight_decay"]), float(group["lr"]) / base))
        if not tensors:
            return loss
        self._state_block(tensors[0][0].device)
        launch = self._table(tensors)
        self._launch(*launch)
        params = [t[0] for t in tensors]
        torch._C._increment_version(params)
        self._dev_pending += 1
        if every:
            self._fast = (params, [t[1] for t in tensors], [p.data_ptr() for p in params], self._hyper(), launch)
        return loss
