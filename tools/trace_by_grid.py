#!/usr/bin/env python
"""Per-dispatch summary of a rocprofv3 kernel trace: one row per (kernel, grid, workgroup) instead of one per kernel name, so that
launches of one kernel at different shapes (the three set-abstraction levels of the inference path) are told apart.

    python tools/trace_by_grid.py <..._kernel_trace.csv> [--match sa_infer] [--skip N] > summary.csv

--skip N drops the first N dispatches of every row (warm-up launches: code-object load, cold caches and clocks)."""
import argparse
import csv
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--match", default="", help="only kernels whose name contains this")
    ap.add_argument("--skip", type=int, default=0)
    args = ap.parse_args()
    rows = {}
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            if args.match not in r["Kernel_Name"]:
                continue
            key = (r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Workgroup_Size_X"])
            rows.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    w = csv.writer(sys.stdout)
    w.writerow(["Name", "Grid_Size_X", "Grid_Size_Y", "Workgroup_Size_X", "Calls", "MedianNs", "MinNs", "MaxNs"])
    for key, ns in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
        ns = ns[args.skip:] or ns
        w.writerow([*key, len(ns), int(statistics.median(ns)), min(ns), max(ns)])


if __name__ == "__main__":
    main()
