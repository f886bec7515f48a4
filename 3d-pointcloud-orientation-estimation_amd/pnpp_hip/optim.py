"""Step glue on ONE flat parameter / gradient buffer.

The reference's loops call opt.zero_grad(), loss.backward(), [clip_grad_norm_], opt.step() over ~60 small
tensors (train_single_peak_vonMises_KL.py:80-85, train_multi_peaks_vonMises_KL.py:221-236).  Here every
parameter is a view into one contiguous buffer and every .grad a view into another, so zero_grad is one
memset, the optimiser one kernel launch, and data parallelism one all-reduce.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from . import _lib as L
from .ops import _stream

MAX_GROUPS = L.PNPP_OPTIM_MAX_GROUPS


class Schedule:
    """A learning-rate schedule the update evaluates on the device from its own step count (csrc/lr_schedule.h): an optional linear
    warm-up from start_factor to 1 over `warmup` updates, then constant, cosine down to min_factor at update `total`, or a factor
    `gamma` every `every` updates, floored at min_factor.  factor(s) is the multiplier of the base rate at the update that follows s
    completed ones -- torch's SequentialLR(LinearLR, CosineAnnealingLR | StepLR) at scheduler epoch s."""

    KINDS = {"constant": L.SCHED_CONSTANT, "cosine": L.SCHED_COSINE, "step": L.SCHED_STEP}

    def __init__(self, kind: str, warmup: int = 0, total: Optional[int] = None, every: int = 0, start_factor: float = 1.0 / 3,
                 min_factor: float = 0.0, gamma: float = 1.0):
        if kind not in self.KINDS:
            raise ValueError(f"Schedule: unknown kind {kind!r} (constant, cosine, step)")
        self.kind, self.warmup, self.total, self.every = kind, int(warmup), None if total is None else int(total), int(every)
        self.start_factor, self.min_factor, self.gamma = float(start_factor), float(min_factor), float(gamma)
        if self.warmup < 0:
            raise ValueError("Schedule: warmup must not be negative")
        if not (0.0 <= self.start_factor <= 1.0 and 0.0 <= self.min_factor <= 1.0):
            raise ValueError("Schedule: start_factor and min_factor must lie in [0, 1]")
        if kind == "cosine" and self.total is not None and self.total <= self.warmup:
            raise ValueError("Schedule: a cosine schedule needs total > warmup")
        if kind == "step" and (self.every < 1 or not 0.0 < self.gamma <= 1.0):
            raise ValueError("Schedule: a step schedule needs every >= 1 and gamma in (0, 1]")

    @classmethod
    def constant(cls, warmup: int = 0, start_factor: float = 1.0 / 3) -> "Schedule":
        return cls("constant", warmup=warmup, start_factor=start_factor)

    @classmethod
    def cosine(cls, total: Optional[int] = None, warmup: int = 0, start_factor: float = 1.0 / 3, min_factor: float = 0.0) -> "Schedule":
        """total=None: to be filled in by the caller that knows the run's length (trainer.fit: epochs x steps per epoch)."""
        return cls("cosine", warmup=warmup, total=total, start_factor=start_factor, min_factor=min_factor)

    @classmethod
    def step(cls, every: int, gamma: float, warmup: int = 0, start_factor: float = 1.0 / 3, min_factor: float = 0.0) -> "Schedule":
        return cls("step", warmup=warmup, every=every, gamma=gamma, start_factor=start_factor, min_factor=min_factor)

    def needs_total(self) -> bool:
        return self.kind == "cosine" and self.total is None

    def with_total(self, total: int) -> "Schedule":
        d = self.to_dict()
        d["total"] = int(total)
        return Schedule(**d)

    def to_dict(self) -> Dict:
        return dict(kind=self.kind, warmup=self.warmup, total=self.total, every=self.every, start_factor=self.start_factor,
                    min_factor=self.min_factor, gamma=self.gamma)

    def fill(self, d: "L.OptimDesc") -> None:
        if self.needs_total():
            raise ValueError("Schedule: a cosine schedule needs `total` before it is used")
        d.sched_kind, d.warmup, d.total, d.every = self.KINDS[self.kind], self.warmup, self.total or 0, self.every
        d.start_factor, d.min_factor, d.gamma = self.start_factor, self.min_factor, self.gamma

    def factor(self, steps_taken: int) -> float:
        """The library's own evaluation (pnpp_lr_factor: host arithmetic, the function the kernel calls)."""
        d, out = L.OptimDesc(), ctypes.c_double()
        self.fill(d)
        L.check(L.lib().pnpp_lr_factor(ctypes.byref(d), int(steps_taken), ctypes.byref(out)))
        return out.value


def plan_groups(params, weight_decay: float = 0.0) -> Tuple[List[torch.nn.Parameter], List[int], List[float], List[float]]:
    """-> (parameters in flat-buffer order, exclusive end of each group, learning-rate multipliers, weight decays).

    params: an iterable of parameters -- one group, today's layout -- or a list of dicts {"params": [...], "weight_decay": w,
    "lr_mult": m} (w defaults to `weight_decay`, m to 1).  Groups lie one after the other in the order given, each keeping the order
    of its parameters; parameters that do not require a gradient are left out.  ValueError: a parameter in two groups, a group with
    no parameter left, more than eight groups."""
    params = list(params)
    if params and all(isinstance(g, dict) for g in params):
        groups = [(list(g["params"]), float(g.get("weight_decay", weight_decay)), float(g.get("lr_mult", 1.0))) for g in params]
    elif any(isinstance(g, dict) for g in params):
        raise ValueError("parameter groups and bare parameters cannot be mixed")
    else:
        groups = [(params, float(weight_decay), 1.0)]
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"at most {MAX_GROUPS} parameter groups, got {len(groups)}")
    ordered, ends, mults, decays, seen = [], [], [], [], set()
    for ps, wd, mult in groups:
        ps = [p for p in ps if p.requires_grad]
        if not ps:
            raise ValueError("optimizer got an empty parameter list" if len(groups) == 1 else "optimizer got an empty parameter group")
        for p in ps:
            if id(p) in seen:
                raise ValueError("a parameter appears in more than one parameter group")
            seen.add(id(p))
        if wd < 0 or mult < 0 or not (math.isfinite(wd) and math.isfinite(mult)):
            raise ValueError("weight_decay and lr_mult must be finite and not negative")
        ordered += ps
        ends.append(sum(p.numel() for p in ordered))
        mults.append(mult)
        decays.append(wd)
    return ordered, ends, mults, decays


def decay_groups(model: torch.nn.Module, weight_decay: float) -> List[Dict]:
    """The usual split for decoupled weight decay: tensors with two or more dimensions (conv and linear weights) decay; one-dimensional
    ones (biases, BatchNorm and LayerNorm weights) do not.  -> [decayed group, undecayed group] for FlatAdam / plan_groups."""
    ps = [p for p in model.parameters() if p.requires_grad]
    return [{"params": [p for p in ps if p.ndim >= 2], "weight_decay": float(weight_decay)},
            {"params": [p for p in ps if p.ndim < 2], "weight_decay": 0.0}]


class FlatAdam:
    """torch.optim.Adam(params, lr, betas, eps) semantics (no amsgrad), one fused launch.  With any of weight_decay, parameter groups, a
    schedule or ema_decay it is torch.optim.AdamW (decoupled=True) or Adam(weight_decay=) (decoupled=False) per group, the rate
    following the schedule on the device and an exponential moving average of the weights kept beside them -- still one launch
    (pnpp_adamw_step); without them the launches are the ones it always made."""

    def __init__(self, params: Iterable, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, fused_grads=True, weight_decay=0.0, decoupled=True,
                 schedule: Optional[Schedule] = None, ema_decay: Optional[float] = None):
        """fused_grads: register every parameter's slice of the flat gradient buffer as the destination the
        backward kernels write to directly; autograd then has no per-parameter accumulation kernels to launch.  The
        first use of a parameter after zero_grad()/step() overwrites its slice; any further use in the same window
        (micro-batch accumulation, two passes summed into one loss, shared weights) is detected when its forward pass
        asks for the destination (ops.grad_sink) and goes through autograd's accumulation into the same memory.

        params: parameters, or a list of group dicts (plan_groups; decay_groups(model, wd) makes the usual two).  weight_decay: of
        every group that names none; decoupled: AdamW's p *= 1 - lr wd, else torch.optim.Adam's g += wd p.  schedule: a Schedule.
        ema_decay: keep `ema`, an exponential moving average of the weights updated in the same launch (ema_weights())."""
        self.params, self.group_ends, self.group_lr_mult, self.group_weight_decay = plan_groups(params, weight_decay)
        self.decoupled, self.schedule = bool(decoupled), schedule
        self.ema_decay = float(ema_decay) if ema_decay else 0.0
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError("ema_decay must lie in [0, 1)")
        if schedule is not None and schedule.needs_total():
            raise ValueError("FlatAdam: a cosine schedule needs `total` (trainer.fit fills it in from the run's length)")
        # any of the additions on: every update goes through pnpp_adamw_step; none: the entry points this class always called
        self._scheduled = self._uses_additions()
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FlatAdam runs on the GPU only (no CPU fallback exists in this package)")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        total = sum(p.numel() for p in self.params)
        self.flat_p = torch.empty(total, device=dev, dtype=torch.float32)
        self.flat_g = torch.zeros(total, device=dev, dtype=torch.float32)
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)
        self._views = []
        off = 0
        for p in self.params:
            n = p.numel()
            self.flat_p[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_p[off:off + n].view(p.shape)
            g = self.flat_g[off:off + n].view(p.shape)
            p.grad = g
            if fused_grads:
                p._pnpp_grad_sink = g
            self._views.append(g)
            off += n
        self.step_count = 0
        # step_dev(): [steps taken, ticket, bits of the float64 rate the last pnpp_adamw_step applied, reserved]
        self._step_state = torch.zeros(4, device=dev, dtype=torch.int64)
        self._scratch = torch.empty(1024 * 8 + 8, device=dev, dtype=torch.uint8)
        self._ss = torch.zeros(1, device=dev, dtype=torch.float64)          # sum of squares of flat_g (clip_grad_norm_)
        self._pending_clip: Optional[float] = None
        self.ema = self.flat_p.clone() if self.ema_decay else None
        self._in_ema = False
        self._desc = self._make_desc() if self._scheduled else None

    @property
    def numel(self) -> int:
        return self.flat_p.numel()

    @property
    def n_groups(self) -> int:
        return len(self.group_ends)

    def _uses_additions(self) -> bool:
        return bool(self.schedule is not None or self.ema_decay or self.n_groups > 1 or any(self.group_weight_decay)
                    or any(m != 1.0 for m in self.group_lr_mult))

    def _make_desc(self) -> "L.OptimDesc":
        d = L.OptimDesc()
        d.n_groups, d.decoupled = self.n_groups, int(self.decoupled)
        for j in range(self.n_groups):
            d.end[j], d.lr_mult[j], d.weight_decay[j] = self.group_ends[j], self.group_lr_mult[j], self.group_weight_decay[j]
        (self.schedule or Schedule.constant()).fill(d)
        d.lr, d.beta1, d.beta2, d.eps, d.ema_decay = self.lr, self.betas[0], self.betas[1], self.eps, self.ema_decay
        return d

    def current_lr(self) -> float:
        """The base rate (lr_mult 1) the NEXT update applies: lr x the schedule's factor at the host's step count (a host float; the
        device's own word is `last_lr`)."""
        lr32 = ctypes.c_float(self.lr).value                      # the launches take lr as a float32
        return lr32 * (self.schedule.factor(self.step_count) if self.schedule is not None else 1.0)

    @property
    def last_lr(self) -> torch.Tensor:
        """The float64 rate lr x factor the last pnpp_adamw_step launch applied, as a 0-dim device view of its state word (0 before the
        first one, and for an optimiser with none of the additions); reading it is the caller's sync."""
        return self._step_state[2:3].view(torch.float64)[0]

    def reset_ema(self) -> None:
        """The average starts again from the weights as they stand (after a broadcast or a load that replaced them)."""
        if self.ema is not None:
            self.ema.copy_(self.flat_p)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the parameters ARE the averaged weights (flat_p and ema trade contents, so model.eval(), state_dict()
        and a Predictor built from the model see them); on exit they trade back, bit for bit.  Buffers (BatchNorm running
        statistics) are not parameters and stay live.  No update may run inside."""
        if self.ema is None:
            raise RuntimeError("FlatAdam was built without ema_decay: there are no averaged weights")
        self._swap_ema()
        self._in_ema = True
        try:
            yield self
        finally:
            self._in_ema = False
            self._swap_ema()

    def _swap_ema(self) -> None:
        with torch.no_grad():
            keep = self.flat_p.clone()
            self.flat_p.copy_(self.ema)
            self.ema.copy_(keep)

    def ema_state_dict(self, model: torch.nn.Module) -> Dict[str, torch.Tensor]:
        """model.state_dict() with the averaged weights in place of the parameters: a detached copy."""
        with self.ema_weights():
            return {k: v.detach().clone() for k, v in model.state_dict().items()}

    def state_dict(self) -> Dict:
        """Everything but the parameters themselves (the model's state_dict has those): step count, both moments, the average, the
        hyper-parameters, the group layout, the schedule and the rate word."""
        return {"version": 1, "step_count": self.step_count, "exp_avg": self.exp_avg.detach().clone(),
                "exp_avg_sq": self.exp_avg_sq.detach().clone(), "ema": None if self.ema is None else self.ema.detach().clone(),
                "last_lr_bits": int(self._step_state[2]),
                "hyper": {"lr": self.lr, "betas": list(self.betas), "eps": self.eps, "decoupled": self.decoupled, "ema_decay": self.ema_decay},
                "layout": {"numel": self.numel, "ends": list(self.group_ends), "lr_mult": list(self.group_lr_mult),
                           "weight_decay": list(self.group_weight_decay), "shapes": [list(p.shape) for p in self.params]},
                "schedule": None if self.schedule is None else self.schedule.to_dict()}

    def load_state_dict(self, sd: Dict) -> None:
        """Into an optimiser built over the same parameters in the same groups.  ValueError: a missing key, another numel or layout, an
        average on one side only."""
        for k in ("version", "step_count", "exp_avg", "exp_avg_sq", "ema", "hyper", "layout", "schedule"):
            if k not in sd:
                raise ValueError(f"FlatAdam.load_state_dict: key {k!r} is missing")
        if sd["version"] != 1:
            raise ValueError(f"FlatAdam.load_state_dict: version {sd['version']!r}, expected 1")
        lay, hyp = sd["layout"], sd["hyper"]
        if int(lay["numel"]) != self.numel or any(tuple(t.shape) != (self.numel,) for t in (sd["exp_avg"], sd["exp_avg_sq"])):
            raise ValueError(f"FlatAdam.load_state_dict: {lay['numel']} elements saved, {self.numel} here")
        if list(lay["ends"]) != list(self.group_ends) or [list(s) for s in lay["shapes"]] != [list(p.shape) for p in self.params]:
            raise ValueError("FlatAdam.load_state_dict: the saved group layout is not this optimiser's")
        if (sd["ema"] is None) != (self.ema is None):
            raise ValueError("FlatAdam.load_state_dict: an averaged copy on one side only (ema_decay)")
        self.lr, self.betas, self.eps = float(hyp["lr"]), (float(hyp["betas"][0]), float(hyp["betas"][1])), float(hyp["eps"])
        self.decoupled = bool(hyp["decoupled"])
        if self.ema is not None:
            self.ema_decay = float(hyp["ema_decay"])
            self.ema.copy_(sd["ema"])
        self.group_lr_mult, self.group_weight_decay = [float(x) for x in lay["lr_mult"]], [float(x) for x in lay["weight_decay"]]
        self.schedule = None if sd["schedule"] is None else Schedule(**sd["schedule"])
        self._scheduled = self._uses_additions()
        self._desc = self._make_desc() if self._scheduled else None
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count = int(sd["step_count"])
        self._step_state.copy_(torch.tensor([self.step_count, 0, int(sd.get("last_lr_bits", 0)), 0], dtype=torch.int64))
        self._dev_steps = self.step_count

    def offset_of(self, param: torch.nn.Parameter) -> int:
        """Start of `param` in the flat buffers (parameters keep the order they were passed in)."""
        off = 0
        for p in self.params:
            if p is param:
                return off
            off += p.numel()
        raise KeyError("parameter is not managed by this optimiser")

    def zero_grad(self) -> None:
        """One memset; autograd then accumulates in place into the flat buffer."""
        self.flat_g.zero_()
        for p, g in zip(self.params, self._views):
            if p.grad is not g:
                p.grad = g
        self._release_sinks()

    def _release_sinks(self) -> None:
        """A new accumulation window: the first backward write of every parameter may overwrite again (ops.grad_sink)."""
        for p in self.params:
            p._pnpp_sink_claimed = False
            p._pnpp_sink_shared = False

    def _sumsq(self) -> torch.Tensor:
        """Sum of squares of the flat gradient buffer into a persistent device word (float64); one stream-ordered launch pair."""
        L.check(L.lib().pnpp_sumsq(self.flat_g.data_ptr(), self.flat_g.numel(), self._ss.data_ptr(), self._scratch.data_ptr(),
                                   self._scratch.numel(), _stream()))
        return self._ss

    def grad_norm(self) -> torch.Tensor:
        """L2 norm of the whole gradient as a 0-dim float64 tensor on the device (no host sync)."""
        return self._sumsq().clone().sqrt_()[0]

    def clip_grad_norm_(self, max_norm: float, return_norm: bool = True) -> Optional[torch.Tensor]:
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm) semantics (train_multi_peaks_vonMises_KL.py:235) with no
        host round trip: the sum of squares is reduced on the device now and the NEXT step()/step_dev() reads it there and
        folds min(1, max_norm / (norm + 1e-6)) into its gradient scale (the gradient buffer itself is left untouched --
        the update consumes it once).  Under data parallelism call it after the all-reduce: the norm that is clipped is
        that of grad_scale * flat_g, i.e. of the mean gradient.  Returns the buffer's own L2 norm as a 0-dim float64 device
        tensor (multiply by grad_scale for the mean gradient's); reading it is the caller's sync, not this method's.
        return_norm=False skips that tensor (two small launches) when the caller does not look at the norm."""
        self._sumsq()
        self._pending_clip = float(max_norm)
        return self._ss.sqrt()[0] if return_norm else None

    def _update(self, step, dev: bool, grad_scale: float, zero_grad: bool) -> None:
        """One launch of the update.  step: the host's count, or (dev) the device words; a pending clip_grad_norm_() picks the _clip entry."""
        self._release_sinks()
        clip, self._pending_clip = self._pending_clip, None
        lib, zero = L.lib(), int(bool(zero_grad))
        if self._scheduled:   # always the device's count: the schedule is a function of it
            d = self._desc
            d.grad_scale, d.max_norm, d.zero_grad = float(grad_scale), (0.0 if clip is None else clip), zero
            if clip is not None and not clip > 0.0:
                raise ValueError("clip_grad_norm_: max_norm must be positive")
            L.check(lib.pnpp_adamw_step(ctypes.byref(d), self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.exp_avg.data_ptr(),
                                        self.exp_avg_sq.data_ptr(), None if self.ema is None else self.ema.data_ptr(), self.flat_p.numel(),
                                        self._step_state.data_ptr(), self._ss.data_ptr() if clip is not None else None, _stream()))
            return
        head = (self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                self.flat_p.numel(), step, self.lr, self.betas[0], self.betas[1], self.eps, float(grad_scale))
        if clip is not None:
            L.check((lib.pnpp_adam_step_dev_clip if dev else lib.pnpp_adam_step_clip)(*head, self._ss.data_ptr(), clip, zero, _stream()))
        elif dev:
            L.check(lib.pnpp_adam_step_dev(*head, zero, _stream()))
        else:
            L.check((lib.pnpp_adam_step_zero if zero else lib.pnpp_adam_step)(*head, _stream()))

    def step(self, grad_scale: float = 1.0, zero_grad: bool = False) -> None:
        """zero_grad=True clears the flat gradient buffer in the same launch (the next iteration's zero_grad())."""
        if self._scheduled:
            return self.step_dev(grad_scale, zero_grad)
        self.step_count += 1
        self._update(self.step_count, False, grad_scale, zero_grad)

    def seed_dev_steps(self) -> None:
        """Copies the host step count into the device word step_dev() reads, if they differ (not capturable: call it
        before a capture starts)."""
        if getattr(self, "_dev_steps", None) != self.step_count:
            self._step_state[:2].copy_(torch.tensor([self.step_count, 0], dtype=torch.int64))
            self._dev_steps = self.step_count

    def step_dev(self, grad_scale: float = 1.0, zero_grad: bool = False) -> None:
        """step() with the step count kept in device memory, so the launch can be captured in a hipGraph and replayed
        (pnpp_hip.graph.GraphedStep(fused_optimizer=True)); `zero_grad` clears the flat gradient buffer in the same launch.
        The device count is re-seeded from `step_count` whenever the two disagree (first use, after eager step()s);
        callers that replay a captured step_dev bump `step_count` themselves."""
        if self._in_ema:
            raise RuntimeError("FlatAdam: no update inside ema_weights() (the parameters are the averaged copy there)")
        self.seed_dev_steps()
        self.step_count += 1
        self._dev_steps = self.step_count
        self._update(self._step_state.data_ptr(), True, grad_scale, zero_grad)
