#!/usr/bin/env python
"""The optimiser launch on the MI355X, the existing kernel beside the scheduled one (csrc/optim_sched_kernels.hip):

    python tools/bench_optim.py --out profiles/optim_sched.json

at n = 1,465,922 (PointNetPPVonMises' flat buffer) and 8 x that, alternating windows in one process (tools/bench_inference.py's
windows: back-to-back launches between two events, microseconds per launch; median, min, max over the windows):

  a        pnpp_adam_step_dev
  b        pnpp_adamw_step, every addition off (16 bytes per lane)
  b_scalar the same with the buffers 4 bytes off a 16-byte boundary: the kernel's one-element-per-lane form
  c        two groups with decoupled weight decay and a cosine schedule
  d        c + the averaged weights

Beside each: the algorithmic bytes (28 per element for a .. c: p, g, m, v read, p, m, v written; + 4 for the folded zero_grad, + 8 for the
average) and the share of the HBM peak they imply at the median.  Back-to-back launches of one kernel overlap their launch costs, so the
windowed time approaches the kernel's own; kernel-only times come from a separate profiler run over `--launches K` (no windows, K
launches of each variant).  Numbers to record, not gates."""
import argparse
import ctypes
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_inference import window  # noqa: E402

N_MODEL = 1_465_922
HBM_PEAK = 8.0e12          # bytes / s, MI355X


def variants(n):
    from pnpp_hip import _lib as L
    lib = L.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(n % 1000)

    def bufs(offset, with_ema=False):
        out = []
        for k in range(5 if with_ema else 4):
            t = torch.empty(n + 4, device="cuda")
            t[:] = torch.rand(n + 4, generator=g).cuda() * (1e-3 if k == 1 else 1.0)
            out.append(t[offset:offset + n])
        return out

    def desc(groups, sched, ema):
        d = L.OptimDesc()
        d.n_groups, d.decoupled = len(groups), 1
        for j, (end, mult, wd) in enumerate(groups):
            d.end[j], d.lr_mult[j], d.weight_decay[j] = end, mult, wd
        d.sched_kind, d.warmup, d.total, d.every, d.start_factor, d.min_factor, d.gamma = sched
        d.lr, d.beta1, d.beta2, d.eps, d.grad_scale, d.max_norm, d.ema_decay, d.zero_grad = 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.0, ema, 1
        return d

    off = (L.SCHED_CONSTANT, 0, 0, 0, 1.0, 0.0, 1.0)
    cos = (L.SCHED_COSINE, 1000, 10_000_000, 0, 0.1, 0.01, 1.0)
    two = [(n - n // 240, 1.0, 1e-2), (n, 1.0, 0.0)]            # the model's split: about 1 in 240 elements is one-dimensional

    def old():
        p, gr, m, v = bufs(0)
        st = torch.zeros(4, dtype=torch.int64, device="cuda")
        return lambda: L.check(lib.pnpp_adam_step_dev(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, st.data_ptr(), 1e-3, 0.9,
                                                      0.999, 1e-8, 1.0, 1, s))

    def new(d, offset=0, ema=False):
        b = bufs(offset, ema)
        st = torch.zeros(4, dtype=torch.int64, device="cuda")
        ptrs = [t.data_ptr() for t in b[:4]] + [b[4].data_ptr() if ema else None]
        keep = (b, st, d)
        return lambda: (keep, L.check(lib.pnpp_adamw_step(ctypes.byref(d), *ptrs, n, st.data_ptr(), None, s)))[1]

    return {"a": (old(), 32), "b": (new(desc([(n, 1.0, 0.0)], off, 0.0)), 32), "b_scalar": (new(desc([(n, 1.0, 0.0)], off, 0.0), 1), 32),
            "c": (new(desc(two, cos, 0.0)), 32), "d": (new(desc(two, cos, 0.999), 0, True), 40)}


def measure(n, windows, seconds):
    runs = variants(n)
    for fn, _ in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts, reps = {k: [] for k in runs}, {k: 64 for k in runs}
    for _ in range(windows):
        for k, (fn, _) in runs.items():
            ms, reps[k] = window(fn, seconds, reps[k])
            ts[k].append(ms * 1e3)
    rec = {"n": n}
    for k, (_, per_elem) in runs.items():
        med = statistics.median(ts[k])
        rec[k] = {"median_us": round(med, 2), "min_us": round(min(ts[k]), 2), "max_us": round(max(ts[k]), 2), "bytes": per_elem * n,
                  "hbm_share": round(per_elem * n / (med * 1e-6) / HBM_PEAK, 3)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--launches", type=int, default=0, help="no windows: this many launches of each variant at each size (for a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on an MI355X; no GPU found")
    if args.launches:
        for n in (N_MODEL, 8 * N_MODEL):
            for fn, _ in variants(n).values():
                for _ in range(args.launches):
                    fn()
            torch.cuda.synchronize()
        return
    doc = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "windows": args.windows,
           "window_s": args.seconds, "hbm_peak_bytes_per_s": HBM_PEAK, "sizes": [measure(n, args.windows, args.seconds) for n in (N_MODEL, 8 * N_MODEL)]}
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
