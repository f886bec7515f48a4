#!/usr/bin/env python3
"""Times one training step of the vanilla PointNet (models/pointnet.py, feature_transform=True): forward + MSE + 0.001 x the
feature-transform regulariser + backward + fused Adam, B = 32 clouds of N = 1024 points, captured in one hipGraph and timed
with device events.  Prints one JSON line (clouds/s, ms per step, library launches per step, FLOPs per step from the shapes,
the wide kernel's share of the float32 matrix peak) and, as a side line, the same step as an eager stock-PyTorch float32
restatement (F.conv1d / F.batch_norm on the same state_dict, torch.optim.Adam) on the same GPU.  Not the driver's bench line.

    python tools/bench_pointnet.py [--steps 50] [--warmup 10] [--no-stock]
    python tools/bench_pointnet.py --lengths [--out profiles/pn_ragged.json]

--lengths times the eager training step (forward + loss + backward + fused Adam; a ragged step's row count depends on the data,
so it is not captured) on a RAGGED batch at 32 x 1024 -- DeviceCloudBank.padded(ids) of a bank whose clouds have seeded lengths,
uniform on [N/4, N] -- against the same clouds resampled to N rows (bank.sample(ids, N)) run without lengths.  The two alternate
in one process, in windows; one JSON line (appended to --out) in the format of tools/bench_inference.py --lengths.  The bank hands
out a device lengths tensor, which costs the step one read-back per forward (the packed row count sizes allocations);
`ragged_host_lengths` is the same step given the lengths as a host list, which costs none.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_FP32 = 157.3e12   # MI355X float32 matrix (= vector) peak, FLOP/s


def step_flops(B, N):
    """Forward FLOPs of the per-point products from the shapes (first layers on rows padded to 4 columns), the head and T-Net
    tails, and the three pooled 128 -> 1024 layers alone."""
    M = B * N
    per_point = [(4, 64), (64, 128), (128, 1024),                 # input T-Net
                 (4, 64),                                          # encoder conv1
                 (64, 64), (64, 128), (128, 1024),                 # feature T-Net
                 (64, 64),                                         # x @ trans_feat
                 (64, 128), (128, 1024)]                           # encoder conv2, conv3
    fwd = sum(2 * M * k * c for k, c in per_point)
    tails = [(1024, 512), (512, 256), (256, 9), (1024, 512), (512, 256), (256, 4096), (1024, 512), (512, 256), (256, 3)]
    fwd += sum(2 * B * k * c for k, c in tails)
    wide = 3 * 2 * M * 128 * 1024
    return fwd, wide


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def stock_step(state, x, t):
    """The same model as plain float32 PyTorch (eager), written from the module definitions: returns a step closure."""
    P = {k: v.clone().cuda().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in state.items()}
    params = [v for v in P.values() if v.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3)

    def bn(pre, z):
        return F.batch_norm(z, P[pre + ".running_mean"], P[pre + ".running_var"], P[pre + ".weight"], P[pre + ".bias"], True, 0.1, 1e-5)

    def conv(pre, z):
        return F.conv1d(z, P[pre + ".weight"], P[pre + ".bias"])

    def tnet(pre, z, k):
        z = F.relu(bn(pre + ".bn1", conv(pre + ".conv1", z)))
        z = F.relu(bn(pre + ".bn2", conv(pre + ".conv2", z)))
        z = F.relu(bn(pre + ".bn3", conv(pre + ".conv3", z))).max(2)[0]
        z = F.relu(bn(pre + ".bn4", F.linear(z, P[pre + ".fc1.weight"], P[pre + ".fc1.bias"])))
        z = F.relu(bn(pre + ".bn5", F.linear(z, P[pre + ".fc2.weight"], P[pre + ".fc2.bias"])))
        z = F.linear(z, P[pre + ".fc3.weight"], P[pre + ".fc3.bias"])
        return (z + torch.eye(k, device=z.device).flatten()).view(-1, k, k)

    def forward(xx):
        xx = xx.transpose(1, 2)
        trans = tnet("encoder.stn", xx, 3)
        xx = torch.bmm(xx.transpose(1, 2), trans).transpose(1, 2)
        xx = F.relu(bn("encoder.bn1", conv("encoder.conv1", xx)))
        tf = tnet("encoder.fstn", xx, 64)
        xx = torch.bmm(xx.transpose(1, 2), tf).transpose(1, 2)
        xx = F.relu(bn("encoder.bn2", conv("encoder.conv2", xx)))
        g = bn("encoder.bn3", conv("encoder.conv3", xx)).max(2)[0]
        h = F.relu(bn("bn1", F.linear(g, P["fc1.weight"], P["fc1.bias"])))
        h = F.relu(bn("bn2", F.dropout(F.linear(h, P["fc2.weight"], P["fc2.bias"]), 0.4, True)))
        return F.linear(h, P["fc3.weight"], P["fc3.bias"]), tf

    def step():
        opt.zero_grad()
        out, tf = forward(x)
        reg = (torch.bmm(tf, tf.transpose(1, 2)) - torch.eye(64, device=tf.device)).flatten(1).norm(dim=1).mean()
        (F.mse_loss(out, t) + 0.001 * reg).backward()
        opt.step()

    return step


def ragged_main(args):
    import datetime
    import benchline
    from bench_inference import launches, ragged_bank_batch
    from bench_pt_inference import alternate, ragged_record
    from models.pointnet import PointNet
    from pnpp_hip import ops, optim
    B, N = 32, 1024
    torch.manual_seed(42)
    model = PointNet(True).cuda().train()
    opt = optim.FlatAdam(model.parameters(), lr=1e-3)
    xyz, dev_lengths, lengths, full = ragged_bank_batch(B, N)
    host = [int(n) for n in lengths]
    t = torch.randn(B, 3, generator=torch.Generator().manual_seed(7)).cuda()

    def step(x, L):
        opt.zero_grad()
        out, _, tf = model(x, return_transforms=True, lengths=L)
        (ops.mse_rows(out, t).mean() + 0.001 * ops.feature_transform_regularizer(tf)).backward()
        opt.step()

    runs = {"ragged": lambda: step(xyz, dev_lengths), "resampled": lambda: step(full, None), "ragged_host_lengths": lambda: step(xyz, host)}
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    rec = {"model": "PointNet(feature_transform=True)", "B": B, "N": N, "date": datetime.date.today().isoformat(),
           "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window,
           "workload": "PointNet forward + MSE + 0.001 x regulariser + backward + fused Adam, eager; ragged batch (DeviceCloudBank.padded) "
                       "against every cloud resampled to N rows (DeviceCloudBank.sample)",
           "launches": {k: launches(fn) for k, fn in runs.items()},
           # device time of the library's kernels alone (instrumented, serialised launches): what packing saves on the device
           "kernel_ms_per_step": {k: round(sum(r[2] for r in benchline.profiled_rows(fn, 5)) / 5, 4) for k, fn in runs.items()}}
    line = json.dumps(ragged_record(rec, alternate(runs, args.windows, args.window, 4), lengths, N))
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--lengths", action="store_true", help="the eager step on a ragged batch (seeded lengths, uniform on [N/4, N], from a "
                                                           "DeviceCloudBank) against every cloud resampled to N rows, at 32 x 1024")
    ap.add_argument("--windows", type=int, default=5, help="--lengths: timing windows per path")
    ap.add_argument("--window", type=float, default=0.5, help="--lengths: seconds of device time per window")
    ap.add_argument("--out", default=None, help="--lengths: append the JSON line to this file")
    args = ap.parse_args()
    if args.lengths:
        if not torch.cuda.is_available():
            raise SystemExit("bench_pointnet: no GPU (this measurement has no CPU form)")
        return ragged_main(args)
    import benchline
    import synthetic
    from models.pointnet import PointNet
    from pnpp_hip import ops, optim
    from pnpp_hip.graph import GraphedStep
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointnet: no GPU (this measurement has no CPU form)")
    B, N = 32, 1024
    torch.manual_seed(42)
    model = PointNet(True)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda().train()
    opt = optim.FlatAdam(model.parameters(), lr=1e-3)
    xyz, _, _, fwd = synthetic.rotated_clouds(B, N, seed=1)
    xyz, fwd = xyz.cuda(), fwd.float().cuda()

    def loss_fn(x, t):
        out, _, tf = model(x, return_transforms=True)
        return ops.mse_rows(out, t).mean() + 0.001 * ops.feature_transform_regularizer(tf)

    def eager_step():
        opt.zero_grad()
        loss_fn(xyz, fwd).backward()
        opt.step()

    rows = benchline.profiled_rows(eager_step, 5)                 # library launches, per-kernel device time (eager)
    g = GraphedStep(opt, loss_fn, [xyz, fwd], fused_optimizer=True)
    ms = timed(lambda: g(xyz, fwd), args.steps, args.warmup)
    fwd_flops, wide_flops = step_flops(B, N)
    scan = [r for r in rows if r[0].startswith("pn_pool_scan_kernel")]
    scan_ms = sum(r[2] for r in scan) / 5
    top = rows[0]
    rec = {"metric": "clouds/sec fwd+bwd", "value": B / (ms * 1e-3), "unit": "clouds/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"models.PointNet(feature_transform=True) fwd+MSE+reg+bwd+fused Adam, one hipGraph, B={B} N={N}"},
           "launches_per_step": sum(r[1] for r in rows) / 5,
           "forward_flops_per_step": fwd_flops, "wide_forward_flops_per_step": wide_flops,
           "kernel_ms_per_step": sum(r[2] for r in rows) / 5,
           "dominant_kernel": {"tag": top[0], "ms_per_step": top[2] / 5, "launches_per_step": top[1] / 5},
           "wide_scan": {"ms_per_step": scan_ms, "tflops": wide_flops / (scan_ms * 1e-3) / 1e12,
                         "fraction_of_fp32_matrix_peak": wide_flops / (scan_ms * 1e-3) / PEAK_FP32,
                         "floor_us_at_peak": wide_flops / PEAK_FP32 * 1e6},
           "kernels": [{"tag": t, "launches_per_step": c / 5, "us_per_step": 1e3 * m / 5} for t, c, m in rows[:12]]}
    print(json.dumps(rec))
    if not args.no_stock:
        torch.manual_seed(43)
        sms = timed(stock_step(state, xyz, fwd), args.steps, args.warmup)
        print(json.dumps({"metric": "clouds/sec fwd+bwd (side line)", "value": B / (sms * 1e-3), "unit": "clouds/s",
                          "ms_per_step": sms, "config": {"workload": "the same step as eager stock PyTorch float32 (F.conv1d / "
                                                         "F.batch_norm, torch.optim.Adam), same GPU, same state_dict"},
                          "hip_speedup": sms / ms}))


if __name__ == "__main__":
    main()
