"""Epoch loop shared by the drop-in training scripts (train_single_peak_vonMises_KL.py:73-107,
train_multi_peaks_vonMises_KL.py:194-318, train_8dir_KL.py:78-152).

One step = forward -> loss -> backward -> [flat gradient all-reduce] -> [clip, on the device] -> fused Adam (which also
clears the gradients it consumed: the next iteration's zero_grad()).  When the batch shape is static and nothing in the
step needs the host (centre sampler 'device' or 'fps'), forward + loss + backward are captured once into a hipGraph and
replayed (pnpp_hip.graph.GraphedStep) -- the launch-bound eager path is only taken for a ragged last batch or a
host-side sampler.  The per-step `loss.item()` of the reference (a device sync every step) is replaced by per-sample
losses kept on the device and read once per phase; with them come the reference's per-label curves
(train_8dir_KL.py:103-110, train_multi_peaks_vonMises_KL.py:239-243).  With WORLD_SIZE > 1 every rank trains on its shard.
"""
from __future__ import annotations

import contextlib
import copy
import os
import time
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import dist as pdist
from . import optim


class SyntheticLoader:
    """In-memory stand-in for a DataLoader (the reference ships no dataset): yields device-resident batches, a label
    column (all zeros unless given) last, like the reference's dataset tuples."""

    def __init__(self, tensors, batch, shuffle, device, generator=None, labels=None):
        n = tensors[0].shape[0]
        labels = torch.zeros(n, dtype=torch.int64) if labels is None else labels.to(torch.int64)
        self.tensors = [t.to(device) for t in list(tensors) + [labels]]
        self.batch, self.shuffle, self.gen = batch, shuffle, generator
        self.n = n

    def __len__(self):
        return (self.n + self.batch - 1) // self.batch

    def __iter__(self):
        order = torch.randperm(self.n, generator=self.gen) if self.shuffle else torch.arange(self.n)
        order = order.to(self.tensors[0].device)
        for i in range(0, self.n, self.batch):
            sel = order[i:i + self.batch]
            yield tuple(t[sel] for t in self.tensors)


class AugmentedLoader:
    """Any loader that yields (xyz, *targets, labels), each batch passed through `augment` (pnpp_hip.augment.Augment): one launch
    that turns the clouds and moves the targets along.  kinds: one per target ("angle", "vm", "axis", "dir8", "keep"); the labels
    column is kept.  device: move the batch there first (a host DataLoader); None: the batch is already on the device.
    counts: index of the target that holds the number of real rows of the multi-row "vm" / "angle" targets (the multi-peak K)."""

    def __init__(self, loader, augment, kinds, device=None, counts=None):
        self.loader, self.augment, self.kinds, self.device, self.counts = loader, augment, tuple(kinds) + ("keep",), device, counts

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if len(batch) != len(self.kinds) + 1:
                raise ValueError(f"AugmentedLoader: a batch of {len(batch)} entries, expected xyz, {len(self.kinds) - 1} targets and labels")
            if self.device is not None:
                batch = tuple(b.to(self.device, non_blocking=True) for b in batch)
            yield self.augment(*batch, kinds=self.kinds, counts=None if self.counts is None else batch[1 + self.counts])


class ViewLoader:
    """Any loader that yields (xyz, ...), the first element of each batch passed through `view` (pnpp_hip.views.SingleView): one
    launch that removes what a viewer on one side cannot see.  The cloud is not moved, so the targets stay as they are, and an
    AugmentedLoader goes around this one.  A resampling view (resample=num) yields uniform (B, num, 3) clouds and batches of the
    loader's own layout; a ragged one appends the per-cloud lengths as the batch's last element.  device: move the batch there
    first (a host DataLoader); None: the batch is already on the device."""

    def __init__(self, loader, view, device=None):
        self.loader, self.view, self.device = loader, view, device

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if self.device is not None:
                batch = tuple(b.to(self.device, non_blocking=True) for b in batch)
            seen = self.view(batch[0])
            yield (seen, *batch[1:]) if self.view.resample is not None else (seen[0], *batch[1:], seen[1])


class PrepLoader:
    """Any loader that yields (xyz, ...), the first element of each batch passed through `prep` (pnpp_hip.scans.ScanPrep with
    resample=num): voxel grid, outlier removal and the unit frame on the device, then `num` rows drawn from the survivors, so the
    batches keep the loader's own layout.  Yaw is invariant under the frame, so the targets stay as they are; a ViewLoader and an
    AugmentedLoader go around this one.  device: move the batch there first (a host DataLoader); None: it is already there."""

    def __init__(self, loader, prep, device=None):
        if prep.resample is None:
            raise ValueError("PrepLoader: the preparation needs resample=num, the uniform batch the models take")
        self.loader, self.prep, self.device = loader, prep, device

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if self.device is not None:
                batch = tuple(b.to(self.device, non_blocking=True) for b in batch)
            yield (self.prep(batch[0])[0], *batch[1:])


LossFn = Union[Callable, Tuple[Callable, Callable]]


def _split(loss_fn: LossFn):
    """loss_fn(model, batch) -> (B,) losses, or the pair (forward(model, batch) -> outputs, criterion(outputs, batch) ->
    (B,) losses) when the caller wants the reference's separate forward / loss timing buckets."""
    if isinstance(loss_fn, tuple):
        fwd, crit = loss_fn
        return fwd, crit, (lambda model, batch: crit(fwd(model, batch), batch))
    return None, None, loss_fn


class PhaseTimer:
    """The reference's four wall-clock buckets per batch (train_multi_peaks_vonMises_KL.py:207-237,248-252): data -> device,
    forward, loss, backward + step.  Its host clocks bracket asynchronous launches; here every bucket edge synchronises the
    device so the numbers mean what their names say -- which costs throughput, so it is opt-in (timing=True /
    PNPP_TIMING=1) and forces the eager path (phases of a replayed graph cannot be told apart)."""

    NAMES = ("data", "fwd", "loss", "bwd")

    def __init__(self, on: bool):
        self.on = on
        self.sums = {k: 0.0 for k in self.NAMES}
        self.n = 0
        self._t = 0.0

    def start(self):
        if self.on:
            torch.cuda.synchronize()
            self._t = time.time()

    def lap(self, name):
        if self.on:
            torch.cuda.synchronize()
            now = time.time()
            self.sums[name] += now - self._t
            self._t = now

    def done(self):
        self.n += 1

    def detail(self, train: bool) -> str:
        if not self.on or self.n == 0:
            return ""
        a = {k: v / self.n for k, v in self.sums.items()}
        s = f"(avg/batch: data={a['data'] * 1e3:.2f}ms fwd={a['fwd'] * 1e3:.2f}ms loss={a['loss'] * 1e3:.2f}ms"
        return s + (f" bwd={a['bwd'] * 1e3:.2f}ms)" if train else ")")


class _TrainStep:
    """forward + loss + backward (+ all-reduce, clip) + Adam for one batch; graph replay when it can, eager otherwise."""

    def __init__(self, model, loss_fn: LossFn, opt: optim.FlatAdam, clip_norm: Optional[float], world: int, use_graph: bool,
                 timer: PhaseTimer):
        self.model, self.opt, self.clip_norm, self.world, self.timer = model, opt, clip_norm, world, timer
        self.fwd, self.crit, self.loss_fn = _split(loss_fn)
        self.use_graph = use_graph and not timer.on and self._graphable(model)
        self.graphed, self.key, self.last_key = None, None, None
        self._seeds: Dict[int, torch.Tensor] = {}
        self.graph_steps = self.eager_steps = 0
        opt.zero_grad()                                   # from here on the update clears what it consumed

    @staticmethod
    def _graphable(model) -> bool:
        """A captured step cannot call the host generator: every set-abstraction level must draw its centres on the device."""
        for m in model.modules():
            if getattr(m, "group_all", True) is False and getattr(m, "sampler", "device") == "randperm":
                return False
        return True

    def _seed(self, n: int, device) -> torch.Tensor:
        """d mean(lv) / d lv = 1/n, the tensor loss.backward() would build (train_single_peak_vonMises_KL.py:83-84)."""
        s = self._seeds.get(n)
        if s is None:
            s = torch.full((n,), 1.0 / n, device=device, dtype=torch.float32)
            self._seeds[n] = s
        return s

    def _body(self, *batch) -> torch.Tensor:
        lv = self.loss_fn(self.model, batch)
        torch.autograd.backward([lv], [self._seed(lv.shape[0], lv.device)])
        return lv.detach()

    def _capture(self, batch, device):
        from .graph import GraphedStep
        from . import sampling
        static = [b.to(device).clone() if torch.is_tensor(b) else b for b in batch]
        keep = [b.detach().clone() for b in self.model.buffers()]       # warm-up passes must not count as training steps:
        streams, rng = sampling.snapshot(), torch.cuda.get_rng_state(device)   # running statistics, random streams are put back
        try:
            self.graphed = GraphedStep(self.opt, self._body, static, adopt_inputs=True, zero_grad_in_graph=False)
        except Exception as e:   # capture is an optimisation, never a requirement
            print(f"[trainer] hipGraph capture failed, staying eager: {type(e).__name__}: {e}")
            self.graphed, self.use_graph = None, False
            torch.cuda.synchronize()
        with torch.no_grad():
            for b, k in zip(self.model.buffers(), keep):
                b.copy_(k)
        sampling.restore(streams)
        torch.cuda.set_rng_state(rng, device)
        self.opt.zero_grad()

    def __call__(self, batch: Sequence, device) -> torch.Tensor:
        key = tuple((tuple(b.shape), b.dtype) if torch.is_tensor(b) else None for b in batch)
        if self.use_graph and self.graphed is None and key == self.last_key:   # the second batch of this shape: it is static
            self.key = key
            self._capture(batch, device)
        self.last_key = key
        t = self.timer
        if self.graphed is not None and key == self.key:
            lv = self.graphed(*batch).clone()             # H2D (or D2D) straight into the graph's static inputs, then replay
            self.graph_steps += 1
        else:
            t.start()
            batch = tuple(b.to(device, non_blocking=True) if torch.is_tensor(b) else b for b in batch)
            t.lap("data")
            if self.fwd is not None and t.on:
                out = self.fwd(self.model, batch)
                t.lap("fwd")
                lv = self.crit(out, batch)
                t.lap("loss")
                torch.autograd.backward([lv], [self._seed(lv.shape[0], lv.device)])
                lv = lv.detach()
            else:
                lv = self._body(*batch)
            self.eager_steps += 1
        pdist.all_reduce_flat_grad(self.opt.flat_g)
        if self.clip_norm is not None:                    # norm of the MEAN gradient, on the device (no .item())
            self.opt.clip_grad_norm_(self.clip_norm)
        self.opt.step(grad_scale=1.0 / self.world, zero_grad=True)
        t.lap("bwd")
        t.done()
        return lv


class _PhaseLog:
    """Per-sample losses (device) and labels of one phase; reduced on the host once, at the end of the phase."""

    def __init__(self, n_labels: int):
        self.n_labels = n_labels
        self.lv: List[torch.Tensor] = []
        self.lab: List[torch.Tensor] = []

    def add(self, lv: torch.Tensor, labels: Optional[torch.Tensor]):
        self.lv.append(lv)
        if labels is not None:
            self.lab.append(labels.detach().reshape(-1))

    def reduce(self, device):
        """-> (mean over every rank's samples, per-label means [nan where a label has no sample])."""
        nl = self.n_labels
        pack = np.zeros(2 + 2 * nl)
        if self.lv:
            v = torch.cat(self.lv).double().cpu().numpy()                 # the one device read of the phase
            pack[0], pack[1] = v.sum(), v.size
            if nl and self.lab:
                lab = torch.cat([l.cpu() for l in self.lab]).numpy().astype(np.int64)
                ok = (lab >= 0) & (lab < nl)
                pack[2:2 + nl] = np.bincount(lab[ok], weights=v[ok], minlength=nl)
                pack[2 + nl:] = np.bincount(lab[ok], minlength=nl)
        if pdist.world_size() > 1:   # one tiny all-reduce per epoch and phase: all ranks agree on the history
            import torch.distributed as tdist
            t = torch.from_numpy(pack).to(device)
            tdist.all_reduce(t)
            pack = t.cpu().numpy()
        total = float(pack[0] / max(pack[1], 1.0))
        with np.errstate(invalid="ignore", divide="ignore"):
            per = np.where(pack[2 + nl:] > 0, pack[2:2 + nl] / pack[2 + nl:], np.nan)
        return total, [float(x) for x in per]


def fit(model: torch.nn.Module, loss_fn: LossFn, loaders: Dict[str, Iterable], epochs: int, lr: float,
        device: torch.device, clip_norm: Optional[float] = None, log: Callable = print, label: str = "KL",
        label_index: Optional[int] = None, n_labels: int = 0, use_graph: Optional[bool] = None, timing: Optional[bool] = None,
        weight_decay: float = 0.0, schedule: Optional[optim.Schedule] = None, ema_decay: Optional[float] = None,
        checkpoint=None, resume=None):
    """Trains with FlatAdam; returns (history, best_state, best_val_epoch).

    weight_decay > 0: decoupled (AdamW) decay of every tensor with two or more dimensions (optim.decay_groups).  schedule: an
    optim.Schedule for the rate, evaluated on the device step by step; a cosine without `total` ends at epochs x steps per epoch.
    ema_decay: an exponential moving average of the weights is kept, and the validation phase and best_state use it.  With any of the
    three, hist["lr"] holds the rate of each epoch's last update as the device reported it (the constant lr otherwise).
    checkpoint: a path written after every epoch (save_checkpoint); resume: such a file to continue from -- the run that results is
    the uninterrupted one.

    loss_fn(model, batch) -> per-sample loss vector (B,) on the device (or a (forward, criterion) pair, see _split);
    batch tensors are already on `device` when it is called.  label_index: position of the class-index column in the
    batch tuple (the reference's datasets yield it last); with n_labels > 0 the history also carries
    hist["labels"][i][phase] -- the per-label epoch means the reference scripts plot and summarise.
    best_state is a deep copy taken at the best validation epoch (the reference keeps live references, so its
    "best" checkpoint is in fact the last one -- train_single_peak_vonMises_KL.py:90; the copy is deliberate).
    """
    world = pdist.world_size()
    if world > 1 and os.environ.get("PNPP_SYNC_BN") == "1":
        # SyncBN (off by default): BatchNorm statistics pooled over the ranks, so the global batch normalises like the reference's
        # single process on the concatenated batch (22 small all-reduces per step; DDP-style per-rank statistics otherwise)
        pdist.enable_sync_batchnorm()
        if pdist.dist.get_backend() != "nccl" and use_graph is None:
            use_graph = False                     # a host-staged exchange cannot be captured into a hipGraph
    if use_graph is None:
        use_graph = os.environ.get("PNPP_NO_GRAPH") != "1"
    if timing is None:
        timing = os.environ.get("PNPP_TIMING") == "1"
    if schedule is not None and schedule.needs_total():
        per_epoch = _common_steps(loaders["train"], device)
        schedule = schedule.with_total(epochs * (per_epoch if per_epoch is not None else len(loaders["train"])))
    params = [g for g in optim.decay_groups(model, weight_decay) if g["params"]] if weight_decay else model.parameters()
    opt = optim.FlatAdam(params, lr=lr, schedule=schedule, ema_decay=ema_decay)
    pdist.broadcast_flat(opt.flat_p)
    opt.reset_ema()
    _, _, plain_loss = _split(loss_fn)
    hist = {"train": [], "val": [], "labels": [{"train": [], "val": []} for _ in range(n_labels)], "timing": [],
            "seconds": {"train": [], "val": []}, "samples": {"train": [], "val": []}, "lr": [], "ema": opt.ema is not None}
    best_val, best_state, best_ep, first_ep = float("inf"), None, None, 1
    if resume is not None:
        ck = load_checkpoint(resume, model, opt, device)
        hist, first_ep = ck["hist"], ck["epoch"] + 1
        best_val, best_state, best_ep = ck["best"]
    t0 = time.time()
    train_timer = PhaseTimer(timing)
    step = _TrainStep(model, loss_fn, opt, clip_norm, world, use_graph, train_timer)
    for ep in range(first_ep, epochs + 1):
        ep_t = time.time()
        details = {}
        for phase in ("train", "val"):
            if phase not in loaders:
                continue
            model.train() if phase == "train" else model.eval()
            plog = _PhaseLog(n_labels)
            timer = train_timer if phase == "train" else PhaseTimer(timing)
            if phase == "train":
                timer.sums, timer.n = {k: 0.0 for k in PhaseTimer.NAMES}, 0
            limit = _common_steps(loaders[phase], device) if phase == "train" else None
            ph_t = time.time()
            # validation sees the averaged weights when there are any (and so does the copy kept as best_state)
            with (opt.ema_weights() if phase == "val" and opt.ema is not None else contextlib.nullcontext()):
                for step_i, batch in enumerate(loaders[phase]):
                    if limit is not None and step_i >= limit:
                        break   # every rank takes the same number of optimiser steps (one all-reduce each)
                    labels = batch[label_index] if label_index is not None else None
                    if phase == "train":
                        lv = step(batch, device)
                    else:
                        lv = _eval_batch(model, loss_fn, batch, device, timer)
                    plog.add(lv, labels)
                avg, per = plog.reduce(device)                   # reads the losses back: the phase's work is finished here
                if phase == "train":                             # the rate of the epoch's last update, from the device's own word
                    hist["lr"].append(float(opt.last_lr) if opt._scheduled else float(lr))
                hist["seconds"][phase].append(time.time() - ph_t)
                hist["samples"][phase].append(sum(int(t.shape[0]) for t in plog.lv))
                hist[phase].append(avg)
                for i, v in enumerate(per):
                    hist["labels"][i][phase].append(v)
                details[phase] = timer.detail(phase == "train")
                if phase == "val" and avg < best_val:
                    best_val, best_ep = avg, ep
                    best_state = copy.deepcopy(model.state_dict())
        va = hist["val"][-1] if hist["val"] else float("nan")
        hist["timing"].append(details)
        if checkpoint is not None and pdist.rank() == 0:
            save_checkpoint(checkpoint, model, opt, ep, hist, (best_val, best_state, best_ep), device)
        if pdist.rank() == 0:
            el = time.time() - ep_t
            eta = (time.time() - t0) / ep * (epochs - ep)
            extra = "".join(f" | {ph}: {d}" for ph, d in details.items() if d)
            log(f"Ep {ep:03}/{epochs} Train {hist['train'][-1]:.4f} Val {va:.4f} | {label} | Time: {el:.1f}s | "
                f"ETA: {eta / 60:.1f}m{extra}")
    hist["steps"] = {"graph": step.graph_steps, "eager": step.eager_steps}
    if best_state is None:
        best_state = copy.deepcopy(model.state_dict())
    return hist, best_state, best_ep


def save_checkpoint(path, model, opt: optim.FlatAdam, epoch: int, hist: dict, best=(float("inf"), None, None), device=None) -> None:
    """Everything a run needs to go on as if it had not stopped: the model (parameters and buffers), the optimiser (FlatAdam.state_dict:
    step count, moments, averaged weights, schedule), the epoch just finished, the history, the best validation result so far, the
    device-side random streams (centre sampler, in-kernel dropout) and torch's CPU and device generator states.  Written to a
    temporary file and moved into place, so an interrupted write leaves the previous checkpoint."""
    from . import sampling
    device = opt.flat_p.device if device is None else device
    ck = {"version": 1, "model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "optimizer": _to_cpu(opt.state_dict()),
          "epoch": int(epoch), "hist": copy.deepcopy(hist), "best": (best[0], _to_cpu(best[1]), best[2]),
          "streams": sampling.snapshot_values(), "rng": {"cpu": torch.get_rng_state(), "device": torch.cuda.get_rng_state(device)}}
    tmp = f"{path}.tmp"
    torch.save(ck, tmp)
    os.replace(tmp, path)


def load_checkpoint(path, model, opt: optim.FlatAdam, device=None) -> dict:
    """Puts save_checkpoint's file back into `model` and `opt` (built as for the run that wrote it) and into the random streams;
    -> the checkpoint, for its "epoch", "hist" and "best" = (best_val, best_state, best_epoch)."""
    from . import sampling
    device = opt.flat_p.device if device is None else device
    ck = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(ck, dict) or ck.get("version") != 1 or any(k not in ck for k in ("model", "optimizer", "epoch", "hist", "best")):
        raise ValueError(f"{path}: not a checkpoint of this trainer")
    model.load_state_dict(ck["model"])       # copies into the parameters in place: they stay views of the optimiser's flat buffer
    opt.load_state_dict(ck["optimizer"])
    sampling.restore_values(ck["streams"])
    torch.set_rng_state(ck["rng"]["cpu"])
    torch.cuda.set_rng_state(ck["rng"]["device"], device)
    best_val, best_state, best_ep = ck["best"]
    if best_state is not None:
        best_state = {k: v.to(device) if torch.is_tensor(v) else v for k, v in best_state.items()}
    ck["best"] = (best_val, best_state, best_ep)
    return ck


def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return type(x)((k, _to_cpu(v)) for k, v in x.items())
    return x


def _eval_batch(model, loss_fn: LossFn, batch, device, timer: Optional[PhaseTimer] = None) -> torch.Tensor:
    fwd, crit, plain = _split(loss_fn)
    t = timer if timer is not None else PhaseTimer(False)
    t.start()
    batch = tuple(b.to(device, non_blocking=True) if torch.is_tensor(b) else b for b in batch)
    t.lap("data")
    with torch.no_grad():
        if fwd is not None and t.on:
            out = fwd(model, batch)
            t.lap("fwd")
            lv = crit(out, batch)
            t.lap("loss")
        else:
            lv = plain(model, batch)
    t.done()
    return lv.detach()


def _eval_batch_metrics(model, loss_fn: LossFn, batch, device, metrics, label_index: Optional[int]) -> torch.Tensor:
    """_eval_batch with the model's outputs also decoded into `metrics` (pnpp_hip.decode.AngularErrors): two more launches."""
    fwd, crit, _ = _split(loss_fn)
    if fwd is None:
        raise ValueError("evaluate(metrics=) needs loss_fn as the (forward, criterion) pair: the metrics decode the forward's outputs")
    batch = tuple(b.to(device, non_blocking=True) if torch.is_tensor(b) else b for b in batch)
    with torch.no_grad():
        out = fwd(model, batch)
        lv = crit(out, batch)
        metrics.update_outputs(out, batch, None if label_index is None else batch[label_index])
    return lv.detach()


def evaluate(model, loss_fn: LossFn, loader, device, label_index: Optional[int] = None, n_labels: int = 0, metrics=None):
    """Mean per-sample loss over `loader` (every rank's samples); with n_labels > 0 returns (mean, per-label means).
    metrics: an AngularErrors that every batch's decoded outputs are added to on the device (its summary() is the caller's to
    take); the return value is the same with and without it."""
    model.eval()
    plog = _PhaseLog(n_labels)
    for batch in loader:
        if metrics is not None:
            lv = _eval_batch_metrics(model, loss_fn, batch, device, metrics, label_index)
        else:
            lv = _eval_batch(model, loss_fn, batch, device)
        plog.add(lv, batch[label_index] if label_index is not None else None)
    total, per = plog.reduce(device)
    return (total, per) if n_labels else total


def _common_steps(loader, device):
    """With more than one rank: the smallest number of batches any rank's shard yields (shards differ by at most one
    sample, so at most one batch); None for a single process."""
    if pdist.world_size() <= 1:
        return None
    import torch.distributed as tdist
    n = torch.tensor([len(loader)], dtype=torch.int64, device=device)
    tdist.all_reduce(n, op=tdist.ReduceOp.MIN)
    return int(n.item())


def add_optim_args(ap) -> None:
    """The optimiser options of the training scripts, each with its PNPP_* environment twin as default; all off unless given."""
    env = os.environ.get
    ap.add_argument("--weight-decay", type=float, default=float(env("PNPP_WEIGHT_DECAY", 0.0)),
                    help="decoupled (AdamW) weight decay of conv / linear weights; biases and norm weights are left alone")
    ap.add_argument("--lr-schedule", default=env("PNPP_LR_SCHEDULE", "constant"), choices=["constant", "cosine", "step"],
                    help="after the warm-up: constant, cosine to zero over the run, or x --lr-gamma every --lr-step-every updates")
    ap.add_argument("--warmup", type=int, default=int(env("PNPP_WARMUP", 0)), help="updates of linear warm-up from a third of the rate")
    ap.add_argument("--lr-step-every", type=int, default=int(env("PNPP_LR_STEP_EVERY", 1000)))
    ap.add_argument("--lr-gamma", type=float, default=float(env("PNPP_LR_GAMMA", 0.5)))
    ap.add_argument("--ema", type=float, default=float(env("PNPP_EMA", 0.0)),
                    help="decay of an exponential moving average of the weights, used for validation and the best checkpoint (0: none)")


def optim_kwargs(args) -> dict:
    """add_optim_args's options as fit()'s keyword arguments ({} when all are off: fit then launches what it always did)."""
    kw = {}
    if args.weight_decay:
        kw["weight_decay"] = args.weight_decay
    if args.lr_schedule == "cosine":
        kw["schedule"] = optim.Schedule.cosine(warmup=args.warmup)
    elif args.lr_schedule == "step":
        kw["schedule"] = optim.Schedule.step(args.lr_step_every, args.lr_gamma, warmup=args.warmup)
    elif args.warmup:
        kw["schedule"] = optim.Schedule.constant(warmup=args.warmup)
    if args.ema:
        kw["ema_decay"] = args.ema
    return kw


def add_metrics_args(ap) -> None:
    """--angular-metrics (PNPP_ANGULAR_METRICS=1): decode the test split's predictions on the device and report angular errors."""
    ap.add_argument("--angular-metrics", action="store_true", default=os.environ.get("PNPP_ANGULAR_METRICS", "0") not in ("", "0"),
                    help="after the run: angular errors of the test split (pnpp_hip.decode), printed and written to "
                         "angular_errors.json beside the results; every other output file is unchanged")


def add_prepare_args(ap) -> None:
    """--prepare (PNPP_PREPARE=1): every split's clouds through pnpp_hip.scans.ScanPrep on the device.  Off by default."""
    ap.add_argument("--prepare", action="store_true", default=os.environ.get("PNPP_PREPARE") == "1",
                    help="treat the clouds as raw scans: a 32-cell voxel grid, statistical outlier removal (k=16, 2 sigma) and the unit "
                         "frame on the device, resampled to the loader's point count (every split; in front of --views and --augment)")


def prepared(loaders: dict, num_points: int, seed: int, device=None) -> dict:
    """Every loader of `loaders` behind a PrepLoader of its own (--prepare): test scans are as raw as training scans."""
    from .scans import ScanPrep
    return {k: PrepLoader(v, ScanPrep(grid=32, outlier_k=16, outlier_std=2.0, resample=num_points, seed=seed + i), device)
            for i, (k, v) in enumerate(loaders.items())}


def report_angular_errors(path, summary: dict, names: Optional[Sequence[str]] = None) -> None:
    """Prints an AngularErrors.summary() (overall line, then one per named label) and writes it as JSON to `path`."""
    import json

    def line(tag, e):
        t, c = e["top1"], e["cover"]
        if not e["n"]:
            return f"  {tag}: no sample with an error ({e['excluded']} excluded)"
        return (f"  {tag}: n {e['n']} (+{e['excluded']} excluded) | top-1 mean {t['mean']:.2f} median <= {t['median']:.1f} p90 <= {t['p90']:.1f} deg, "
                f"within 5/10/22.5 deg {t['within_5']:.3f}/{t['within_10']:.3f}/{t['within_22.5']:.3f} | "
                f"cover median <= {c['median']:.1f} p90 <= {c['p90']:.1f} deg | mode count right {e['count_ok_rate']:.3f}")

    print("Angular errors (test split):")
    print(line("overall", summary["overall"]))
    out = dict(summary)
    if names is not None and len(names) == len(summary["labels"]):
        out["label_names"] = list(names)
        for name, e in zip(names, summary["labels"]):
            print(line(name, e))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


def env_path(name: str, default: str):
    from pathlib import Path
    return Path(os.environ.get(name, default))
