#!/usr/bin/env python
"""Surface normals: the fused launch (pnpp_hip.normals.estimate_normals) against the same mathematics from ops.knn plus torch ops.

    python tools/bench_normals.py --out profiles/normals.json

Cases: 32 x 1024 k=16, 256 x 2048 k=32, 16 x 10,000 k=16 (the scripts' own cloud size), clouds uniform in a cube, orient="centroid",
curvature asked for.  One JSON line per case: ms per call of the fused call, of ops.knn alone at S = N (its floor: the same search
without the epilogue) and of the torch side (median over the windows with the min-max spread; the sides alternate in one process, every
window at least --window seconds of back-to-back calls between device events closed by a synchronise), the fused kernel's own time
(events on its dispatch packet, the library's profiler) and the largest angle between the two sides' normals.  There is no speed
target: the figures are recorded as they come.

The torch side: ops.knn, a gather of the neighbours, float64 differences, mean and covariance by einsum, torch.linalg.eigh on the
device, sign and curvature by elementwise ops.  Where this torch build cannot run eigh on the device the line says so ("torch":
null, "torch_error") and the fused call stands beside ops.knn alone.

--lib PATH times another build of the library (a variant of a compile-time constant); --cases 0,2 picks cases by position."""
import argparse
import datetime
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

CASES = ((32, 1024, 16), (256, 2048, 32), (16, 10000, 16))


def torch_normals(x, k):
    from pnpp_hip import normals, ops
    idx = ops.knn(x, x, k).long()
    B, N, _ = x.shape
    p = x.double()
    rows = idx + torch.arange(B, device=x.device)[:, None, None] * N
    nb = p.reshape(B * N, 3)[rows.reshape(-1)].view(B, N, k, 3)
    d = nb - p[:, :, None, :]
    m = d.mean(2)
    C = torch.einsum("bnki,bnkj->bnij", d, d) / k - m[..., :, None] * m[..., None, :]
    w, v = torch.linalg.eigh(C)
    n = v[..., 0]
    big = torch.gather(n, 2, n.abs().argmax(-1, keepdim=True))
    n = torch.where(big < 0, -n, n)
    s = (n * (p - normals.reference_points(x).double()[:, None, :])).sum(-1, keepdim=True)
    n = torch.where(s < 0, -n, n)
    tr = w.sum(-1)
    flat = tr <= 0
    curv = torch.where(flat, torch.zeros_like(tr), w[..., 0].clamp_min(0) / torch.where(flat, torch.ones_like(tr), tr))
    return torch.where(flat[..., None], torch.zeros_like(n), n).float(), curv.float()


def window(fn, seconds, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 1e3 * seconds:
            return ms / reps, reps
        reps = max(reps + 1, int(reps * 1.2e3 * seconds / max(ms, 1e-3)))


def alternate(fns, windows, seconds):
    times, reps = [[] for _ in fns], [1] * len(fns)   # one call first: a side may take seconds per call
    for _ in range(windows):   # alternately: drift of the clocks hits every side alike
        for i, fn in enumerate(fns):
            ms, reps[i] = window(fn, seconds, reps[i])
            times[i].append(ms)
    return [{"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for t in times]


def case(B, N, k, windows, seconds, with_torch=True):
    from benchline import profiled_rows
    from pnpp_hip import normals, ops
    x = torch.rand(B, N, 3, generator=torch.Generator().manual_seed(B + N), dtype=torch.float32).cuda()
    fused = lambda: normals.estimate_normals(x, k, "centroid", curvature=True)
    knn = lambda: ops.knn(x, x, k)
    tor = lambda: torch_normals(x, k)
    for _ in range(3):
        a, _c = fused()
        knn()
    torch.cuda.synchronize()
    rec = {"case": f"{B} x {N} k={k}", "torch": None}
    sides = [fused, knn]
    if with_torch:
        try:
            b, _c = tor()
            torch.cuda.synchronize()
            cross = torch.linalg.cross(a.double(), b.double()).norm(dim=-1)
            rec["max_angle_fused_vs_torch_rad"] = float(cross.max())
            rec["median_angle_fused_vs_torch_rad"] = float(cross.median())
            sides.append(tor)
        except Exception as e:   # this torch build cannot run eigh (or a gather this large) on the device
            rec["torch_error"] = f"{type(e).__name__}: {str(e)[:200]}"
    rows = profiled_rows(fused, 20)
    rec["fused_kernel_us"] = {tag.split()[0]: 1e3 * ms / cnt for tag, cnt, ms in rows}
    t = alternate(sides, windows, seconds)
    rec["fused"], rec["knn_alone_S_eq_N"] = t[0], t[1]
    rec["fused_over_knn_alone"] = t[0]["ms"] / t[1]["ms"]
    if len(t) == 3:
        rec["torch"], rec["speedup_call"] = t[2], t[2]["ms"] / t[0]["ms"]
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="least seconds of back-to-back calls per timed window")
    ap.add_argument("--cases", default=None, help="comma-separated positions in CASES (default: all)")
    ap.add_argument("--lib", default=None, help="time this build of the shared library instead of the in-tree one")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch side (variant sweeps)")
    ap.add_argument("--tag", default=None, help="a label copied into every line (variant sweeps)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals needs the GPU: there is nothing to time without one")
    if args.lib:
        from pnpp_hip import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    stamp = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "windows": args.windows,
             "window_s": args.window}
    if args.tag:
        stamp["tag"] = args.tag
    picked = CASES if args.cases is None else [CASES[int(i)] for i in args.cases.split(",")]
    lines = [dict(case(B, N, k, args.windows, args.window, not args.no_torch), **stamp) for B, N, k in picked]
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "a" if args.tag else "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
