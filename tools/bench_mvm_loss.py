#!/usr/bin/env python
"""The mixture KL on the decode grid (ops.mvm_grid_kl: one launch, value and gradients), forward + backward, against the same mathematics
written with torch ops on the device, and beside ops.match_loss.

    python tools/bench_mvm_loss.py --out profiles/mvm_grid_kl.json

Cases: 32 x K=4 and 256 x K=4 mixtures (tools/bench_decode.py's: kappa log-uniform on [0.5, 80], Dirichlet weights), num = 360.  One
JSON line per case: ms per forward + backward of every side (median over the windows, min-max spread; the sides alternate in one
process, every window at least --window seconds of back-to-back calls between device events closed by a synchronise), the kernel's own
time (events attached to its dispatch packet, the library's profiler), launches per call, and the largest difference between the HIP
and the torch side.  There is no speed target: the figures are recorded as they come.

The torch side: float64, the log-density of both mixtures on the grid by one broadcast expression and logsumexp each, the rectangle
rule, torch autograd for the gradients.  A call of each side is the loss of every sample, its sum, and the gradient with respect to mu,
kappa and weight (leaf tensors), as a training step would ask for.
"""
import argparse
import datetime
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_decode import alternate, mixtures, torch_launches  # noqa: E402

TWO_PI = 2.0 * math.pi


class TorchSide:
    """KL(ground truth || prediction) on the grid in torch ops, float64, no host synchronisation."""

    def __init__(self, num=360):
        self.G = num - 1
        self.theta = torch.arange(self.G, dtype=torch.float64, device="cuda") * (TWO_PI / self.G)

    def log_mix(self, mu, kappa, logw):   # (B, K) each -> (B, G)
        lv = kappa[:, :, None] * (torch.cos(self.theta[None, None, :] - mu[:, :, None]) - 1.0)
        lv = lv - torch.log(TWO_PI * torch.special.i0e(kappa))[:, :, None]
        return torch.logsumexp(lv + logw[:, :, None], dim=1)

    def __call__(self, mu, kappa, weight, vm_gt, K_gt):
        gt = vm_gt.double()
        used = (torch.arange(gt.size(1), device="cuda")[None, :] < K_gt[:, None]) & (gt[:, :, 2] > 0)
        v = torch.where(used, gt[:, :, 2], torch.zeros_like(gt[:, :, 2]))
        logv = torch.where(used, torch.log(v / v.sum(1, keepdim=True)), torch.full_like(v, -float("inf")))
        lq = self.log_mix(gt[:, :, 0], gt[:, :, 1].clamp(0.0, 500.0), logv)
        lp = self.log_mix(mu.double(), kappa.double().clamp(0.0, 500.0), torch.log(weight.double()))
        return ((TWO_PI / self.G) * (torch.exp(lq) * (lq - lp)).sum(1)).float()


def case(B, K, num, windows, seconds):
    from benchline import profiled_rows
    from pnpp_hip import ops
    mu, kappa, weight, vm_gt, K_gt = mixtures(B, K, 7 + B)
    leaves = [t.clone().requires_grad_(True) for t in (mu, kappa, weight)]
    g = torch.Generator().manual_seed(B)
    raws = [t.cuda().requires_grad_(True) for t in (torch.randn(B, K, generator=g), torch.randn(B, 2 * K, generator=g),
                                                    torch.randn(B, K, generator=g))]
    ts = TorchSide(num)

    def both(loss_of, wrt):
        def run():
            loss = loss_of()
            return (loss, *torch.autograd.grad(loss.sum(), wrt))
        return run

    hip = both(lambda: ops.mvm_grid_kl(*leaves, vm_gt, K_gt, num), leaves)
    head = both(lambda: ops.mvm_head_grid_kl(*raws, vm_gt, K_gt, 0.7, 80.0, num), raws)
    tor = both(lambda: ts(*leaves, vm_gt, K_gt), leaves)
    match = both(lambda: ops.match_loss(*leaves, vm_gt, K_gt), leaves)
    for _ in range(5):
        a, b = hip(), tor()
        head(), match()
    torch.cuda.synchronize()
    rel = [float(((x.double() - y.double()).abs() / y.double().abs().clamp_min(1e-30))[y.abs() > 1e-6 * y.abs().max()].max()) for x, y in zip(a, b)]
    rows = profiled_rows(hip, 50)
    kernels = {tag.split()[0]: {"launches_per_call": cnt / 50, "us": 1e3 * ms / cnt} for tag, cnt, ms in rows}
    rows_h = profiled_rows(head, 50)
    kernels.update({tag.split()[0]: {"launches_per_call": cnt / 50, "us": 1e3 * ms / cnt} for tag, cnt, ms in rows_h})
    t_hip, t_head, t_tor, t_match = alternate((hip, head, tor, match), windows, seconds)
    return {"case": f"mvm_grid_kl forward + backward {B} x K={K} num={num}", "hip": t_hip, "hip_head_form": t_head, "torch": t_tor,
            "match_loss": t_match, "hip_kernels": kernels, "torch_launches_per_call": torch_launches(tor),
            "hip_launches_per_call": torch_launches(hip), "speedup_call": t_tor["ms"] / t_hip["ms"],
            "max_rel_diff_hip_vs_torch_float32": dict(zip(("loss", "dmu", "dkappa", "dweight"), rel))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds of back-to-back calls per timed window")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvm_loss needs the GPU: there is nothing to time without one")
    stamp = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "windows": args.windows,
             "window_s": args.window}
    lines = [dict(case(B, 4, 360, args.windows, args.window), **stamp) for B in (32, 256)]
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
