#!/usr/bin/env python3
"""Per-launch table of the replayed step from a rocprofv3 kernel trace, for judging a store policy (pnpp_set_store_policy) launch by launch:
    rocprofv3 --kernel-trace -d <dir> -o t --output-format csv -- python3 bench.py --steps 200 --warmup 20 --no-cpu-baseline --no-roofline --no-bf16-variant --no-mfma-variant
    python tools/store_policy_table.py <dir>                                 # the table as text
    python tools/store_policy_table.py <dir> <session> <variant> <out.csv>   # ... and appended to a csv, one row per launch
    python tools/store_policy_table.py --from-csv <csv> <session> <variant>  # the text table again from such a csv
The last 100 steps (a step ends with the Adam launch).  Per position in the step, over those replays:
    dur   duration of the launch
    s2s   start of this launch -> start of the next
    span  start of this launch -> END of the next (= s2s + the next launch's duration): what a flush paid at the boundary, or a slower
          first read in the consumer, cannot hide from.  mean, min and max; a policy pays at a launch when the means differ by more
          than the min-max spread.
    MB    bytes the launch writes, from the shapes of the flagship step (32 clouds x 1024 points): its output arrays | its partial slabs
          (dW partials, float64 statistics, moment partials), to 0.1 MB"""
import collections
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from summarize_rocprof import any_tag  # noqa: E402

# MB written per launch of the flagship step, in launch order: (kernel name prefix, output arrays, partial slabs).  Rows M: sa1 131072,
# sa2 32768, sa3 1024, head 32.  Outputs: M x N x 4 (+ the pooled extremes and arg-max rows where the epilogue pools); slabs: workers x K x
# N x 4 of dW, workers x 2 x N x 8 of statistics.  A step with other launches prints no byte counts.
STEP_WRITES = [
    ("knn_pair_kernel", 0.7, 0.1), ("gemm_wsf03_kernel", 33.6, 0.5), ("bn_finalize_fwd_kernel", 0.0, 0.0), ("gemm_wsf3_kernel<64", 71.3, 0.5),
    ("bn_finalize_fwd_kernel", 2.1, 0.0), ("gemm_smallm_kernel", 2.1, 0.0), ("gather_rel_stats_kernel", 16.8, 1.0),
    ("bn_finalize_fwd_kernel", 0.0, 0.0), ("gemm_wsf3_kernel<128", 16.8, 0.3), ("bn_finalize_fwd_kernel", 0.0, 0.0),
    ("gemm_wsf3_kernel<128", 35.7, 0.3), ("bn_finalize_fwd_kernel", 1.0, 0.0), ("gemm_smallm_kernel", 1.0, 0.1),
    ("bn_finalize_fwd_kernel", 0.0, 0.0), ("gemm_smallm_kernel", 2.1, 0.3), ("bn_finalize_fwd_kernel", 0.0, 0.0),
    ("gemm_mid3_kernel", 4.5, 0.3), ("bn_finalize_fwd_kernel", 0.1, 0.0), ("gemm_smallm_kernel", 0.1, 0.0), ("gemm_smallm_kernel", 0.1, 0.0),
    ("vm_fc_head_kl_step_kernel", 0.1, 0.0), ("fc_bwd_fused_kernel", 0.6, 0.0), ("fc_bwd_fused_kernel", 2.2, 0.0),
    ("bn_finalize_bwd_kernel", 4.2, 0.0), ("da_dw_mid_kernel", 4.2, 0.1), ("post_gemm_kernel", 2.1, 0.0), ("da_dw_kernel", 1.0, 16.9),
    ("post_gemm_kernel", 1.5, 0.0), ("da_dw_kernel", 1.0, 10.5), ("slab_reduce_kernel", 0.3, 0.0), ("pool_bwd_kernel", 1.0, 0.3),
    ("bn_finalize_bwd_kernel", 0.0, 0.0), ("gemm_wsd3_kernel<256", 16.8, 8.5), ("post_gemm_kernel", 0.1, 0.0),
    ("gemm_wsd3_kernel<128,32,A4", 16.8, 4.3), ("post_gemm_kernel", 0.1, 0.0), ("scatter_dz_kernel", 2.1, 0.3), ("da_dw_kernel", 2.1, 8.4),
    ("slab_reduce2_kernel", 0.1, 0.0), ("pool_bwd_kernel", 2.1, 0.5), ("bn_finalize_bwd_kernel", 0.0, 0.0),
    ("gemm_wsd3_kernel<128,32,A5", 33.6, 4.3), ("post_gemm_kernel", 0.1, 0.0), ("gemm_wsx_kernel", 0.0, 4.7), ("xyz0_post_kernel", 0.1, 0.0),
    ("adam_kernel", 17.5, 0.0),
]
HEADER = ["session", "variant", "wall_us_per_step", "pos", "kernel_and_grid", "dur_us", "start_to_start_us", "span_us", "span_min_us", "span_max_us"]


def writes(names):
    """(MB out, MB slab) per position, or blanks when the step is not the flagship's"""
    if len(names) != len(STEP_WRITES) or any(not names[p].startswith(w[0]) for p, w in enumerate(STEP_WRITES)):
        return [("", "")] * len(names)
    return [(w[1], w[2]) for w in STEP_WRITES]


def show(wall, rows):
    """rows: (pos, name, dur, s2s, span, span_min, span_max) as strings"""
    w = writes([r[1] for r in rows])
    print(f"# {len(rows)} launches per step, wall {wall} us per step over the last 100 replays; times in us")
    print(f"# {'pos':>3} {'dur':>7} {'s2s':>7} {'span':>7} {'span_min':>8} {'span_max':>8} {'MB out':>7} {'MB slab':>7}  kernel")
    for r, (mo, ms) in zip(rows, w):
        print(f"  {int(r[0]):3d} {r[2]:>7} {r[3]:>7} {r[4]:>7} {r[5]:>8} {r[6]:>8} {mo:>7} {ms:>7}  {r[1]}")


def main():
    if sys.argv[1] == "--from-csv":
        rows = [r for r in csv.DictReader(open(sys.argv[2])) if r["session"] == sys.argv[3] and r["variant"] == sys.argv[4]]
        show(rows[0]["wall_us_per_step"], [(r["pos"], r["kernel_and_grid"], r["dur_us"], r["start_to_start_us"], r["span_us"], r["span_min_us"],
                                            r["span_max_us"]) for r in rows])
        return
    f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = []
    for r in csv.DictReader(open(f)):
        wg = int(r.get("Workgroup_Size_X", 256) or 256)
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                     any_tag(r["Kernel_Name"], int(r["Grid_Size_X"]), int(r.get("Grid_Size_Y", 1) or 1), wg)))
    rows.sort()
    ends = [i for i, r in enumerate(rows) if "adam_kernel" in r[2]]
    steps = 100
    bounds = ends[-steps - 1:]
    n = bounds[1] - bounds[0]
    assert all(b - a == n for a, b in zip(bounds, bounds[1:])), "the replayed steps differ in their launch count"
    per = collections.defaultdict(lambda: ([], [], []))
    names = {}
    for a in bounds[:-1]:
        for p in range(n):
            s, e, name = rows[a + 1 + p]
            ns, ne, _ = rows[a + 2 + p] if a + 2 + p < len(rows) else (e, e, "")
            names[p] = name
            d = per[p]
            d[0].append((e - s) / 1e3), d[1].append((ns - s) / 1e3), d[2].append((ne - s) / 1e3)
    wall = f"{(rows[bounds[-1]][1] - rows[bounds[0]][1]) / steps / 1e3:.1f}"
    m = lambda v: sum(v) / len(v)
    out = [(str(p), names[p], f"{m(per[p][0]):.2f}", f"{m(per[p][1]):.2f}", f"{m(per[p][2]):.2f}", f"{min(per[p][2]):.2f}", f"{max(per[p][2]):.2f}")
           for p in range(n)]
    show(wall, out)
    if len(sys.argv) > 4:
        new = not os.path.exists(sys.argv[4])
        with open(sys.argv[4], "a", newline="") as fo:
            wr = csv.writer(fo)
            if new:
                wr.writerow(HEADER)
            for r in out:
                wr.writerow([sys.argv[2], sys.argv[3], wall] + list(r))


if __name__ == "__main__":
    main()
