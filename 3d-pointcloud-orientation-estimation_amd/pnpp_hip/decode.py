"""From von-Mises parameters to orientations, and from orientations to angular-error statistics.

    ori = decode(mu, kappa, weight)              # one launch: the modes of each sample's mixture density (pnpp_mvm_decode)
    errs = AngularErrors(n_labels=10)
    errs.update(ori, vm_gt=vm_gt, K_gt=K_gt, labels=labels)   # one launch, no synchronisation (pnpp_orient_eval)
    errs.summary()                               # ONE read-back (and, with more than one rank, one integer all-reduce)

The accumulator lives on the device as 64-bit integers that the kernel adds to with atomics: the words do not depend on the order
of the additions, so a summary is bit-reproducible.  Everything here is forward-only and usable inside torch.cuda.graph.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from . import dist as pdist
from . import ops

BINS, STRIDE, BIN_DEG = L.ORIENT_BINS, L.ORIENT_STRIDE, 0.5
_INCLUDED, _EXCLUDED, _COUNT_OK, _SUM_TOP1, _SUM_COVER = (2 * BINS + i for i in range(5))
WITHIN_DEG = (5.0, 10.0, 22.5)


class Orientation(NamedTuple):
    angle: torch.Tensor                 # (B,)   the highest mode, radians in (-pi, pi]; NaN where the density is flat
    modes: torch.Tensor                 # (B, K) by descending height; NaN in unused slots
    heights: torch.Tensor               # (B, K) unnormalised density at the modes; 0 in unused slots
    n_modes: torch.Tensor               # (B,)   int32
    density: Optional[torch.Tensor]     # (B, num - 1) the normalised grid density, when asked for


def decode(mu, kappa, weight=None, counts=None, num: int = 360, rel_height: float = 0.1, density: bool = False) -> Orientation:
    """The modes of p(theta) = sum_k weight_k vonMises(theta; mu_k, kappa_k) per sample.  mu, kappa, weight (B,K), K <= 8, or
    mu, kappa (B,) with weight None for the single-peak model; counts (B,): the components in use.  Candidates are the local maxima
    on the grid of num - 1 angles (the reference's mvm_density_on_grid grid), refined to ~1e-8 rad; modes below rel_height x the
    highest are dropped."""
    modes, heights, n_modes, angle, dens = ops.mvm_decode(mu, kappa, weight, counts, num, rel_height, density)
    return Orientation(angle, modes, heights, n_modes, dens)


# ---- histogram -> statistics: pure host code -------------------------------------------------------------------------------
def _hist_stats(hist: np.ndarray, sum_udeg: int) -> dict:
    """Statistics of one error from its histogram of 0.5 degree bins and the sum of the errors in micro-degrees.
    median / p90: the UPPER edge of the first bin at which the cumulative count reaches half / nine tenths of n (rounded up), so the
    true quantile lies within the 0.5 degrees below the figure; within_X: the share of samples in bins that end at or below X degrees
    (exact: 5, 10 and 22.5 are bin edges)."""
    hist = np.asarray(hist, dtype=np.int64)
    n = int(hist.sum())
    if n == 0:
        return {"mean": None, "median": None, "p90": None, **{f"within_{d:g}": None for d in WITHIN_DEG}}
    cum = np.cumsum(hist)

    def quantile(num, den):
        need = -(-n * num // den)   # ceil(n * num / den), at least 1
        return float((int(np.searchsorted(cum, max(need, 1))) + 1) * BIN_DEG)

    out = {"mean": sum_udeg / 1e6 / n, "median": quantile(1, 2), "p90": quantile(9, 10)}
    for d in WITHIN_DEG:
        out[f"within_{d:g}"] = float(hist[:int(round(d / BIN_DEG))].sum() / n)
    return out


def summarize(acc, n_labels: int) -> dict:
    """The accumulator's words (n_labels * STRIDE + 1 integers, any sequence type) -> {"overall": {...}, "labels": [{...}] * n_labels,
    "samples": n}.  Each entry: n (samples with an error), excluded, count_ok_rate (over n + excluded) and, under "top1" and "cover",
    mean / median / p90 in degrees and the accuracies within 5 / 10 / 22.5 degrees; None where there is no sample."""
    acc = np.asarray(acc).astype(np.int64).reshape(-1)
    if acc.size != n_labels * STRIDE + 1:
        raise ValueError(f"accumulator of {acc.size} words, expected n_labels * {STRIDE} + 1 = {n_labels * STRIDE + 1}")
    blocks = acc[:-1].reshape(n_labels, STRIDE)

    def entry(blk):
        n, exc, ok = int(blk[_INCLUDED]), int(blk[_EXCLUDED]), int(blk[_COUNT_OK])
        return {"n": n, "excluded": exc, "count_ok_rate": ok / (n + exc) if n + exc else None,
                "top1": _hist_stats(blk[:BINS], int(blk[_SUM_TOP1])), "cover": _hist_stats(blk[BINS:2 * BINS], int(blk[_SUM_COVER]))}

    return {"overall": entry(blocks.sum(axis=0)), "labels": [entry(b) for b in blocks], "samples": int(acc[-1])}


class AngularErrors:
    """Device-resident angular-error statistics.  update() is one launch and never synchronises; summary() reads back once.
    capacity: rows of the per-sample buffer (`sample_errors()`); samples beyond it still count in the statistics."""

    def __init__(self, n_labels: int = 1, capacity: int = 0, device=None):
        if not 1 <= int(n_labels) <= L.ORIENT_MAX_LABELS:
            raise ValueError(f"n_labels={n_labels} (1 <= n_labels <= {L.ORIENT_MAX_LABELS})")
        if int(capacity) < 0:
            raise ValueError(f"capacity={capacity} must not be negative")
        self.n_labels, self.capacity = int(n_labels), int(capacity)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"AngularErrors on '{self.device}': the pnpp HIP operators run on an AMD GPU only "
                               "(no CPU fallback exists in this package)")
        self.acc = torch.zeros(self.n_labels * STRIDE + 1, dtype=torch.int64, device=self.device)
        self.errors = torch.full((self.capacity, 2), -1.0, device=self.device) if self.capacity else None

    def update(self, orientation: Orientation, mu_gt=None, kappa_gt=None, vm_gt=None, K_gt=None, labels=None) -> None:
        """Adds a batch: ground truth as (mu_gt, kappa_gt) (B,) or (vm_gt (B,Kmax,3), K_gt (B,)); labels (B,) in 0..n_labels-1."""
        ops.orient_eval(orientation.modes, orientation.n_modes, orientation.angle, mu_gt, kappa_gt, vm_gt, K_gt, labels, self.n_labels,
                        self.acc, self.errors, per_sample=False)

    def update_outputs(self, out, batch, labels=None) -> None:
        """A model's outputs and the batch they came from, in the training scripts' layouts: out = (mu, kappa) with
        batch = (xyz, mu_gt, kappa_gt, ...) or (xyz, vm_gt (B,2), ...) for the single-peak model, out = (mu, kappa, weight) with batch = (xyz, vm_gt, K_gt, ...)
        for the multi-peak model.  Two launches: decode and update."""
        if len(out) == 2 and batch[1].dim() == 2:   # the single-peak script's table of (mu, kappa) rows
            self.update(decode(out[0], out[1]), mu_gt=batch[1][:, 0], kappa_gt=batch[1][:, 1], labels=labels)
        elif len(out) == 2:
            self.update(decode(out[0], out[1]), mu_gt=batch[1], kappa_gt=batch[2], labels=labels)
        elif len(out) == 3:
            self.update(decode(out[0], out[1], out[2]), vm_gt=batch[1], K_gt=batch[2], labels=labels)
        else:
            raise TypeError(f"outputs of {len(out)} tensors: expected (mu, kappa) or (mu, kappa, weight)")

    def reset(self) -> None:
        self.acc.zero_()
        if self.errors is not None:
            self.errors.fill_(-1.0)

    def counts(self) -> np.ndarray:
        """The accumulator on the host, summed over the ranks: the one read-back."""
        acc = self.acc
        if pdist.world_size() > 1:
            acc = pdist.sum_over_ranks(acc.clone())
        return acc.cpu().numpy()

    def summary(self) -> dict:
        return summarize(self.counts(), self.n_labels)

    def sample_errors(self) -> torch.Tensor:
        """(n, 2) this rank's per-sample (top1, cover) in degrees, in the order of the updates; -1 for an excluded sample."""
        if self.errors is None:
            raise ValueError("AngularErrors was built with capacity=0: no per-sample buffer")
        return self.errors[:min(int(self.acc[-1].item()), self.capacity)]
