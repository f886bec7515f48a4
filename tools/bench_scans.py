#!/usr/bin/env python
"""The raw-scan preparation steps (pnpp_voxel_downsample, pnpp_outlier_statistic / _filter behind ops.knn, pnpp_normalize_clouds) and
their chain (pnpp_hip.scans.ScanPrep) on the MI355X:

    python tools/bench_scans.py --out profiles/scans.json

At 32 x 2,048 (a training batch) and 16 x 100,000 (raw scans, grid=32), alternating in the same windows (tools/bench_views.py's): each
step alone, the chain with resample=1024, and the same mathematics written with torch ops on the device (floor / unique /
scatter_reduce amin / stable sort for the voxel grid, cdist + topk for the outliers).  At 100,000 rows the outlier step is timed on the
voxel step's output, as the chain runs it -- the search is brute force over the padded width.  Microseconds per call (median, min, max
over the windows: host and device together, back to back calls) and each kernel's own device time from the event pair attached to its
dispatch; --trace FILE adds what a `rocprofv3 --kernel-trace` run of this script (with --trace-run) wrote to its CSV.
One JSON document.  Numbers to record, not gates."""
import argparse
import csv
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_augment import kernel_us, timed  # noqa: E402

CASES = ((32, 2048), (16, 100000))
GRID, K, STD, NUM = 32, 8, 1.0, 1024
KERNELS = ("voxel_clear_kernel", "voxel_bounds_kernel", "voxel_insert_kernel", "voxel_compact_kernel", "outlier_statistic_kernel",
           "outlier_filter_kernel", "normalize_clouds_kernel")


def scans(B, N):
    """surfaces of flattened spheres, twice as dense on one half, 5 % uniform strays, anywhere and of any size"""
    g = torch.Generator().manual_seed(B)
    v = torch.randn(B, N, 3, generator=g)
    v = v / v.norm(dim=2, keepdim=True)
    flip = (v[..., 0] < 0) & (torch.rand(B, N, generator=g) < 0.5)
    v[..., 0] = torch.where(flip, -v[..., 0], v[..., 0])
    v = v * torch.tensor([1.0, 0.6, 0.3])
    stray = torch.rand(B, N, generator=g) < 0.05
    v[stray] = torch.rand(int(stray.sum()), 3, generator=g) * 4 - 2
    return (v * (0.5 + 1.5 * torch.rand(B, 1, 1, generator=g)) + 10 * torch.rand(B, 1, 3, generator=g) - 5).cuda()


def _compact(xyz, mask):
    B, N, _ = xyz.shape
    order = torch.sort((~mask).to(torch.uint8), dim=1, stable=True).indices               # survivors first, in their order
    kept = mask.sum(1)
    out = torch.gather(xyz, 1, order[..., None].expand(-1, -1, 3))
    return out * (torch.arange(N, device=xyz.device)[None, :] < kept[:, None])[..., None], kept.to(torch.int32)


def torch_voxel(xyz, grid):
    """The voxel step with stock torch ops (torch.unique reads its size back); not bit-equal, the same amount of mathematics."""
    B, N, _ = xyz.shape
    lo, hi = xyz.amin(1, keepdim=True), xyz.amax(1, keepdim=True)
    h = ((hi - lo).amax(2, keepdim=True) / grid).clamp_min(1e-30)
    c = ((xyz - lo) / h).floor().clamp_(0, grid - 1)
    d = ((xyz - (lo + (c + 0.5) * h)) ** 2).sum(-1)
    ci = c.long()
    ids = ci[..., 0] | (ci[..., 1] << 10) | (ci[..., 2] << 20) | (torch.arange(B, device=xyz.device)[:, None] << 30)
    key = (d.view(torch.int32).long() << 32) | torch.arange(N, device=xyz.device)
    uniq, inv = torch.unique(ids, return_inverse=True)
    best = torch.full((uniq.numel(),), torch.iinfo(torch.int64).max, device=xyz.device).scatter_reduce_(0, inv.flatten(), key.flatten(), "amin")
    return _compact(xyz, best[inv] == key)


def torch_outliers(xyz, lengths, k, std_ratio):
    B, N, _ = xyz.shape
    valid = torch.arange(N, device=xyz.device)[None, :] < lengths[:, None]
    d = torch.cdist(xyz, xyz).masked_fill(~valid[:, None, :], float("inf"))
    s = d.topk(k + 1, largest=False).values.double().sum(-1) / k
    s = torch.where(valid, s, 0.0)
    mean = s.sum(1) / lengths
    std = (torch.where(valid, (s - mean[:, None]) ** 2, 0.0).sum(1) / lengths).sqrt()
    return _compact(xyz, valid & (s <= (mean + std_ratio * std)[:, None]))


def torch_normalize(xyz, lengths):
    valid = (torch.arange(xyz.shape[1], device=xyz.device)[None, :] < lengths[:, None])[..., None]
    c = (torch.where(valid, xyz, 0.0).double().sum(1) / lengths[:, None]).float()
    q = torch.where(valid, xyz - c[:, None], 0.0)
    return q / q.norm(dim=2).amax(1)[:, None, None], c


def cases(windows, seconds):
    from pnpp_hip import ops
    from pnpp_hip.scans import ScanPrep
    out = []
    for B, N in CASES:
        xyz = scans(B, N)
        vox, vlen = ops.voxel_downsample(xyz, grid=GRID)
        width = N if N <= 4096 else 1 << int(vlen.max()).bit_length()                     # the torch outlier step cannot hold (N, N) at 100,000
        vox_t, full = vox[:, :width].contiguous(), torch.full((B,), N, device="cuda", dtype=torch.int32)
        chain = ScanPrep(grid=GRID, outlier_k=K, outlier_std=STD, resample=NUM, seed=1)
        runs = {"voxel": lambda: ops.voxel_downsample(xyz, grid=GRID),
                "outliers_after_voxel": lambda: ops.remove_outliers(vox, K, STD, vlen),
                "normalize": lambda: ops.normalize_clouds(xyz),
                "scan_prep": lambda: chain(xyz),
                "torch_voxel": lambda: torch_voxel(xyz, GRID),
                "torch_outliers_after_voxel": lambda: torch_outliers(vox_t, vlen, K, STD),
                "torch_normalize": lambda: torch_normalize(xyz, full)}
        if N <= 4096:
            runs["outliers"] = lambda: ops.remove_outliers(xyz, K, STD)
            runs["torch_outliers"] = lambda: torch_outliers(xyz, full, K, STD)
        for fn in runs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        rec = {"case": f"{B} x {N} x 3 flattened shells, one half twice as dense, 5 % strays; grid {GRID}, k {K}, std_ratio {STD}, resample {NUM}",
               "voxel_kept_mean": round(float(vlen.float().mean()), 1), "voxel_kept_max": int(vlen.max()),
               "torch_outliers_after_voxel_width": width,
               "scan_prep_survivors_mean": round(float(chain.last_lengths.float().mean()), 1)}
        rec.update(timed(runs, windows, seconds))
        rec["kernel_us"] = {k: kernel_us(runs["scan_prep"], k, calls=50) for k in KERNELS}
        rec["kernel_us"]["knn (in scan_prep)"] = kernel_us(runs["scan_prep"], "knn", calls=50)
        out.append(rec)
    return out


def trace_run(calls=20):
    """What a rocprofv3 --kernel-trace run of its own executes: the chain's launches and nothing else."""
    from pnpp_hip.scans import ScanPrep
    for B, N in CASES:
        xyz = scans(B, N)
        chain = ScanPrep(grid=GRID, outlier_k=K, outlier_std=STD, resample=NUM, seed=1)
        for _ in range(calls):
            chain(xyz)
    torch.cuda.synchronize()


def read_trace(path):
    """rocprofv3's kernel-trace CSV -> per new kernel and grid size the mean duration in microseconds."""
    by = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = next((k for k in KERNELS if k in row.get("Kernel_Name", "")), None)
            if name:
                key = f"{name} grid {row.get('Grid_Size_X') or row.get('Grid_Size')}x{row.get('Grid_Size_Y') or 1}"
                by.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v), "mean_us": round(sum(v) / len(v), 2), "min_us": round(min(v), 2)} for k, v in sorted(by.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true", help="only launch the chain (the program of a rocprofv3 --kernel-trace run)")
    ap.add_argument("--trace", default=None, help="kernel-trace CSV of such a run, folded into the document")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scans.py measures on an MI355X; no GPU found")
    if args.trace_run:
        return trace_run()
    doc = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "windows": args.windows,
           "window_s": args.seconds, "cases": cases(args.windows, args.seconds)}
    if args.trace:
        doc["rocprofv3_kernel_trace_us"] = read_trace(args.trace)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
