#!/usr/bin/env python
"""Yaw symmetry: the library call (pnpp_hip.symmetry.yaw_symmetry) against the same mathematics in torch ops on the device.

    python tools/bench_symmetry.py --out profiles/symmetry.json

Cases: 32 x 1024 at 72 and at 360 angles; boxes, tapered boxes, square prisms and cylinders in turn, drawn from torch's generator.
One JSON line per case: ms per call of the library call (centroid, two launches, the decision included) and of the torch side (median
over the windows with the min-max spread; the sides alternate in one process, every window at least --window seconds of back-to-back
calls between device events closed by a synchronise), the two kernels' own times (events on their dispatch packets, the library's
profiler, in a pass of its own), the distance evaluations per second that makes, and the largest relative difference between the two
sides' profiles.  There is no speed target: the figures are recorded as they come.

The torch side: centre, then per angle rotate, torch.cdist against the unrotated cloud, square, min over candidates, float64 mean --
one (B, N, N) matrix at a time, G + 1 of them per call (the floor masks the diagonal); S, score and the decision are not formed.

--trace-only N makes N library calls per case and nothing else: what a `rocprofv3 --kernel-trace --stats -- python
tools/bench_symmetry.py --trace-only 20` run of its own traces (the two cases differ in the profile kernel's grid)."""
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

from bench_normals import alternate  # noqa: E402

CASES = ((32, 1024, 72), (32, 1024, 360))


def clouds(B, N, seed):
    """(B, N, 3): boxes, tapered boxes, square prisms and cylinders in turn, each at a random yaw and offset."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(B, N, 3, generator=g) * 2 - 1
    kind = torch.arange(B) % 4
    half = torch.tensor([[0.6, 0.3, 1.0], [0.6, 0.3, 1.0], [0.8, 0.3, 0.8], [0.8, 0.3, 0.8]])[kind]
    p = u * half[:, None, :]
    taper = 0.4 + 0.6 * (p[:, :, 2] + 1.0) / 2.0
    p[:, :, 0] = torch.where((kind == 1)[:, None], p[:, :, 0] * taper, p[:, :, 0])
    r, a = 0.8 * torch.sqrt((u[:, :, 0] + 1) / 2), math.pi * (u[:, :, 2] + 1)
    cyl = (kind == 3)[:, None]
    p[:, :, 0], p[:, :, 2] = torch.where(cyl, r * torch.cos(a), p[:, :, 0]), torch.where(cyl, r * torch.sin(a), p[:, :, 2])
    th = torch.rand(B, generator=g) * 2 * math.pi
    c, s = torch.cos(th)[:, None], torch.sin(th)[:, None]
    x, z = c * p[:, :, 0] + s * p[:, :, 2], c * p[:, :, 2] - s * p[:, :, 0]
    return (torch.stack([x, p[:, :, 1], z], -1) + (torch.rand(B, 1, 3, generator=g) - 0.5)).contiguous()


def torch_profile(x, table):
    from pnpp_hip.normals import reference_points
    c = reference_points(x)
    q = torch.stack([x[:, :, 0] - c[:, None, 0], x[:, :, 1], x[:, :, 2] - c[:, None, 2]], -1)
    B, N, _ = q.shape
    D = torch.empty(B, table.shape[0], device=x.device)
    for g in range(table.shape[0]):
        cs, sn = table[g, 0], table[g, 1]
        rot = torch.stack([cs * q[:, :, 0] + sn * q[:, :, 2], q[:, :, 1], cs * q[:, :, 2] - sn * q[:, :, 0]], -1)
        D[:, g] = torch.cdist(rot, q).square().min(-1).values.double().mean(-1).float()
    d = torch.cdist(q, q).square()
    d.diagonal(dim1=1, dim2=2).fill_(math.inf)
    return D, d.min(-1).values.double().mean(-1).float()


def case(B, N, G, windows, seconds):
    from benchline import profiled_rows
    from pnpp_hip import symmetry
    x = clouds(B, N, B + N + G).cuda()
    lib = lambda: symmetry.yaw_symmetry(x, num=G)
    tor = lambda: torch_profile(x, symmetry.grid_table(G, x.device))
    for _ in range(3):
        a = lib()
    b = tor()
    torch.cuda.synchronize()
    rec = {"case": f"{B} x {N} x {G}", "orders": a.order.tolist(),
           "max_rel_diff_distance": float(((a.profile.distance - b[0]).abs()[:, 1:] / b[0][:, 1:]).max()),
           "max_rel_diff_floor": float(((a.profile.floor - b[1]).abs() / b[1]).max())}
    rows = profiled_rows(lib, 20)
    rec["kernel_us"] = {tag.split()[0]: 1e3 * ms / cnt for tag, cnt, ms in rows}
    evals = B * (G + 1) * N * N
    rec["distance_evaluations"] = evals
    rec["evaluations_per_s_profile_kernel"] = evals / (1e-6 * rec["kernel_us"]["yaw_profile_kernel"])
    t = alternate([lib, tor], windows, seconds)
    rec["library"], rec["torch"], rec["speedup_call"] = t[0], t[1], t[1]["ms"] / t[0]["ms"]
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="least seconds of back-to-back calls per timed window")
    ap.add_argument("--trace-only", type=int, default=0, help="N library calls per case under an external tracer, no timing")
    ap.add_argument("--cases", default=None, help="comma-separated positions in CASES (default: all)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_symmetry needs the GPU: there is nothing to time without one")
    stamp = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "windows": args.windows,
             "window_s": args.window}
    picked = CASES if args.cases is None else [CASES[int(i)] for i in args.cases.split(",")]
    if args.trace_only:
        from pnpp_hip import symmetry
        for B, N, G in picked:
            x = clouds(B, N, B + N + G).cuda()
            for _ in range(args.trace_only):
                symmetry.yaw_symmetry(x, num=G)
            torch.cuda.synchronize()
        return
    lines = [dict(case(B, N, G, args.windows, args.window), **stamp) for B, N, G in picked]
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
