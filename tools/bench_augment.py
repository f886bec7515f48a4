#!/usr/bin/env python
"""The augmentation launch (pnpp_augment_clouds: yaw about +Y per cloud, single-peak target moved along) on the MI355X:

    python tools/bench_augment.py --out profiles/augment.json

  - the fused launch against the same maths written with torch ops on the device (random angle, cos, sin, building R, einsum, the
    wrapped target), at 32 x 1024 and 256 x 2048, the two alternating in the same windows (tools/bench_inference.py's windows):
    microseconds per batch (median, min, max over the windows: host and device together, back to back calls), the launches of
    each, and the fused kernel's own device time;
  - one eager training step of PointNetPPVonMises at 32 x 1024 fed by a BankLoader with augmentation against the same loader
    without, alternating: the time the augmentation adds to a step.
One JSON document.  Numbers to record, not gates."""
import argparse
import datetime
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_inference import launches, window  # noqa: E402


def timed(fns, windows, seconds):
    """fns: {name: callable}, timed alternately -> {name: {"median_us", "min_us", "max_us"}}"""
    ts, reps = {k: [] for k in fns}, {k: 8 for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            ms, reps[k] = window(fn, seconds, reps[k])
            ts[k].append(ms * 1e3)
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in ts.items()}


def torch_launches(fn):
    """Device kernels one call of fn launches, from torch's profiler (None where the profiler reports no device events)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    return n or None


def kernel_us(fn, tag, calls=200):
    """Mean device time of the library launches whose tag starts with `tag`, from the event pair attached to each dispatch
    (pnpp_profile_enable): the kernel's own begin to end, without the host's share of a call."""
    import ctypes
    from pnpp_hip import _lib
    lib = _lib.lib()
    fn()
    torch.cuda.synchronize()
    lib.pnpp_profile_enable(1)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.pnpp_profile_report(buf, len(buf))
    lib.pnpp_profile_enable(0)
    n, ms = 0, 0.0
    for line in buf.value.decode().splitlines():
        parts = line.split("\t")
        if len(parts) >= 3 and parts[0].startswith(tag):
            n, ms = n + int(parts[1]), ms + float(parts[2])
    return round(1e3 * ms / n, 2) if n else None


def torch_yaw(xyz, vm):
    """The augmentation with stock torch ops: the maths of synthetic.rotated_clouds on the device, target wrapped into [-pi, pi)."""
    B = xyz.shape[0]
    th = torch.rand(B, device=xyz.device) * (2 * math.pi)
    c, s = torch.cos(th), torch.sin(th)
    R = torch.zeros(B, 3, 3, device=xyz.device)
    R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = c, s, 1.0, -s, c
    out = torch.einsum("bnj,bij->bni", xyz, R)
    mu = torch.remainder(vm[:, 0] - th + math.pi, 2 * math.pi) - math.pi
    return out, torch.stack([mu, vm[:, 1]], 1)


def launch_cases(windows, seconds):
    from pnpp_hip.augment import Augment
    out = []
    for B, N in ((32, 1024), (256, 2048)):
        g = torch.Generator().manual_seed(B)
        xyz = (torch.rand(B, N, 3, generator=g) * 2 - 1).cuda()
        vm = torch.stack([(torch.rand(B, generator=g) * 2 - 1) * math.pi, torch.full((B,), 8.0)], 1).cuda()
        aug = Augment(seed=1)
        runs = {"fused": lambda: aug(xyz, vm, kinds=("vm",)), "torch_ops": lambda: torch_yaw(xyz, vm)}
        for fn in runs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        rec = {"case": f"{B} x {N} x 3, single-peak target (B, 2)", "bytes_moved": 2 * 4 * B * N * 3,
               "launches": {"fused": launches(runs["fused"]), "torch_ops": torch_launches(runs["torch_ops"])}}
        rec.update(timed(runs, windows, seconds))
        rec["fused"]["kernel_us"] = kernel_us(runs["fused"], "augment_clouds_kernel")
        full = Augment(seed=1, scale=(0.8, 1.25), jitter=(0.01, 0.05))          # float64 Box-Muller per point on top
        rec["fused_yaw_scale_jitter_kernel_us"] = kernel_us(lambda: full(xyz, vm, kinds=("vm",)), "augment_clouds_kernel")
        out.append(rec)
    return out


def step_case(windows, seconds, B=32, N=1024, clouds=256):
    import dataloader_common as dc
    import synthetic
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    from pnpp_hip import ops, optim, sampling
    from pnpp_hip.augment import Augment
    torch.manual_seed(0)
    sampling.reset(0)
    xyz, mu, kappa, _ = synthetic.rotated_clouds(clouds, 2 * N, seed=3)
    vm = torch.stack([mu, kappa], 1)
    model = PointNetPPVonMises(sampler="device").cuda().train()
    opt = optim.FlatAdam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    seed = torch.full((B,), 1.0 / B, device="cuda")

    def endless(**kw):
        loader = dc.BankLoader(dc.DeviceCloudBank(list(xyz.numpy()), "cuda", seed=5), [vm], N, B, True, seed=6, drop_last=True, **kw)
        while True:
            yield from loader

    def step(batches):
        x, t = next(batches)
        lv = ops.vm_head_kl_loss(model.features(x), t[:, 0].contiguous(), t[:, 1].contiguous(), reduction="none")
        torch.autograd.backward([lv], [seed])
        opt.step(grad_scale=1.0, zero_grad=True)

    plain, augmented = endless(), endless(augment=Augment(seed=7), kinds=("vm",))
    runs = {"bank_loader": lambda: step(plain), "bank_loader_augmented": lambda: step(augmented)}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rec = {"case": f"PointNetPPVonMises eager step (draw, forward, fused head + KL, backward, FlatAdam) at {B} x {N}",
           "launches": {k: launches(fn) for k, fn in runs.items()}}
    rec.update(timed(runs, windows, seconds))
    rec["added_us_per_step"] = round(rec["bank_loader_augmented"]["median_us"] - rec["bank_loader"]["median_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on an MI355X; no GPU found")
    doc = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "windows": args.windows,
           "window_s": args.seconds, "launch": launch_cases(args.windows, args.seconds), "step": step_case(args.windows, args.seconds)}
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
