#!/usr/bin/env python3
"""Writes tests/golden/pointnet_pp_cls.npz: the reference's own PointNet++ classifier (PointNet++Demo.py of the reference checkout,
loaded by path) on seeded weights and inputs -- 8 clouds of 1024 points with normals, the reference's level sizes (512 / 0.2 / 32,
128 / 0.4 / 64, whole cloud), 40 classes.  Runs on a CPU box that has the reference:

    python tools/make_golden_pointnet_pp_cls.py /path/to/reference

The index decisions are taken by the reference's own functions in float32 (farthest_point_sample with the start indices it draws
itself after torch.manual_seed, query_ball_point) and recorded; the model then runs in float64 on exactly those indices, train mode,
explicit dropout keep-masks: log-probabilities, nll loss, per-parameter sampled gradients and norms, the running statistics after
the step and the eval-mode log-probabilities after it.  Also recorded: the state_dict's names and shapes and the parameter count.

The case's seed is the first of a list for which every discrete decision is safe under float32 rounding:
  - at each farthest-point step the largest distance leads the second largest by FPS_MARGIN of its value (float32 forms a
    squared distance of three differences to about 2e-7 of its value),
  - no squared centre-to-point distance lies within RADIUS_MARGIN (relative) of a squared radius,
  - every ReLU input of the two 8-row head blocks is RELU_MARGIN away from 0.
The margins found are printed."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pointnet_pp_cls.npz")
B, N, CLASSES, P_DROP, NSAMP = 8, 1024, 40, 0.4, 8
FPS_MARGIN, RADIUS_MARGIN, RELU_MARGIN = 1e-6, 5e-7, 3e-5


def load_ref(ref_root):
    spec = importlib.util.spec_from_file_location("ref_pointnet_pp_demo", os.path.join(ref_root, "PointNet++Demo.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _Mask(nn.Module):
    def __init__(self, mask, p):
        super().__init__()
        self.mask, self.scale = mask, 1.0 / (1.0 - p)

    def forward(self, x):   # nn.Dropout's contract: the identity in eval mode
        return x * self.mask.to(x) * self.scale if self.training else x


def fps_margin(xyz, idx):
    """smallest relative lead of the chosen point over the runner-up along the recorded run (float64); the run must be float64's own too"""
    xyz = xyz.double()
    dist = torch.full(xyz.shape[:2], 1e10, dtype=torch.float64)
    rows = torch.arange(xyz.shape[0])
    worst = float("inf")
    for i in range(idx.shape[1] - 1):
        c = xyz[rows, idx[:, i]].unsqueeze(1)
        dist = torch.minimum(dist, ((xyz - c) ** 2).sum(-1))
        top = dist.topk(2, dim=1)
        if not torch.equal(top.indices[:, 0], idx[:, i + 1]):
            return -1.0
        worst = min(worst, float(((top.values[:, 0] - top.values[:, 1]) / top.values[:, 0]).min()))
    return worst


def radius_margin(xyz, new_xyz, radius):
    d = ((new_xyz.double().unsqueeze(2) - xyz.double().unsqueeze(1)) ** 2).sum(-1)
    return float(((d - radius ** 2).abs() / radius ** 2).min())


def positions(p, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, p.numel(), (min(NSAMP, p.numel()),), generator=g).numpy()


def run_case(ref, seed, out):
    """-> (fps margin, radius margin, relu margin); the later ones are None when an earlier one already rules the seed out"""
    torch.manual_seed(seed)
    model = ref.PointNetPlusPlusCls(num_classes=CLASSES, normal_channel=True)
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(B, 6, N, generator=g)                       # coordinates and "normals" in the unit cube
    target = torch.randint(0, CLASSES, (B,), generator=g)
    masks = [(torch.rand(B, c, generator=g) < 1.0 - P_DROP).to(torch.float64) for c in (512, 256)]

    # the index decisions, by the reference's own float32 functions; its FPS draws the start itself (torch.randint, host generator)
    xyz = x[:, :3].transpose(1, 2).contiguous()
    torch.manual_seed(2000 + seed)
    levels, cur = [], xyz
    for sa in (model.sa1, model.sa2):
        fps = ref.farthest_point_sample(cur, sa.npoint)
        new_xyz = ref.index_points(cur, fps)
        nbr = ref.query_ball_point(sa.radius, sa.nsample, cur, new_xyz)
        levels.append(dict(fps=fps, nbr=nbr, xyz=cur, new_xyz=new_xyz, radius=sa.radius))
        cur = new_xyz
    mf = min(fps_margin(l["xyz"], l["fps"]) for l in levels)
    if mf < FPS_MARGIN:
        return mf, None, None
    mr = min(radius_margin(l["xyz"], l["new_xyz"], l["radius"]) for l in levels)
    if mr < RADIUS_MARGIN:
        return mf, mr, None

    # the float64 run on those indices
    queue = {"fps": [l["fps"] for l in levels], "nbr": [l["nbr"] for l in levels]}
    calls = {"fps": 0, "nbr": 0}

    def replay(kind):
        def fn(*a, **k):
            i = calls[kind] % 2
            calls[kind] += 1
            return queue[kind][i]
        return fn

    own = ref.farthest_point_sample, ref.query_ball_point, F.relu
    margin = [float("inf")]

    def relu(t, inplace=False):
        if t.dim() == 2:
            margin[0] = min(margin[0], float(t.detach().abs().min()))
        return own[2](t, inplace=inplace)

    ref.farthest_point_sample, ref.query_ball_point, F.relu = replay("fps"), replay("nbr"), relu
    try:
        model = model.double().train()
        model.dropout1, model.dropout2 = _Mask(masks[0], P_DROP), _Mask(masks[1], P_DROP)
        logp = model(x.double())
        loss = ref.get_loss()(logp, target)
        loss.backward()
        relu_margin = margin[0]
        if relu_margin < RELU_MARGIN:
            return mf, mr, relu_margin
        after = {k: v.float().numpy() for k, v in model.state_dict().items() if "running" in k}
        model.eval()
        with torch.no_grad():
            ev = model(x.double())
    finally:
        ref.farthest_point_sample, ref.query_ball_point, F.relu = own

    out["seed"], out["x"], out["target"] = np.array(seed), x.numpy(), target.numpy().astype(np.int32)
    out["mask1"], out["mask2"] = (m.to(torch.uint8).numpy() for m in masks)
    for i, l in enumerate(levels, 1):
        out[f"start{i}"] = l["fps"][:, 0].numpy().astype(np.int32)
        out[f"fps{i}"], out[f"nbr{i}"] = l["fps"].numpy().astype(np.int16), l["nbr"].numpy().astype(np.int16)
    out["logp"], out["loss"] = logp.detach().numpy(), np.array(float(loss.detach()))
    for i, (n, p) in enumerate(model.named_parameters()):
        pos = positions(p, i)
        out[f"gp.{n}"] = pos
        out[f"gs.{n}"] = p.grad.detach().flatten()[pos].numpy()
        out[f"gn.{n}"] = np.array(float(p.grad.detach().norm()))
    for k, v in after.items():
        out[f"after.{k}"] = v
    out["eval_logp"] = ev.numpy()
    sd = model.state_dict()
    out["sd.names"] = np.array(list(sd.keys()))
    out["sd.shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    out["n_params"] = np.array(sum(p.numel() for p in model.parameters()))
    return mf, mr, relu_margin


def main():
    ref = load_ref(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PNPP_REFERENCE", "../reference"))
    torch.set_num_threads(8)
    for seed in range(100, 500):
        out = {}
        mf, mr, mrelu = run_case(ref, seed, out)
        print(f"seed {seed}: FPS lead {mf:.2e} of the distance (>= {FPS_MARGIN:.0e})"
              + ("" if mr is None else f", radius gap {mr:.2e} of r^2 (>= {RADIUS_MARGIN:.0e})")
              + ("" if mrelu is None else f", min |ReLU input| of the 8-row blocks {mrelu:.2e} (>= {RELU_MARGIN:.0e})"))
        if out:
            np.savez_compressed(OUT, **{f"cls.{k}": v for k, v in out.items()})   # one case, tagged like the PointNet fixture's
            print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
            return
    raise SystemExit("no seed with float32-safe decisions")


if __name__ == "__main__":
    main()
