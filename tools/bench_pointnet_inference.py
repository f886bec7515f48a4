#!/usr/bin/env python
"""Forward-only throughput of the vanilla PointNet: model.eval() under no_grad against pnpp_hip.Predictor, timed alternately in
one process (window() / launches() of tools/bench_inference.py).

    python tools/bench_pointnet_inference.py                  # PointNet(True), PointNet(False) at B=32 N=1024; PointNet(True) at B=256
    python tools/bench_pointnet_inference.py --out profiles/pointnet_inference_forward.json
    python tools/bench_pointnet_inference.py --trace-only 20  # ~20 Predictor forwards of PointNet(True), B=32 N=1024, and nothing else
    python tools/bench_pointnet_inference.py --lengths --out profiles/pn_ragged.json   # appends one line

--lengths times the Predictor of PointNet(True) on a RAGGED batch at 32 x 1024 -- DeviceCloudBank.padded(ids), seeded lengths uniform
on [N/4, N] -- against the same clouds resampled to N rows (bank.sample(ids, N)) run without lengths, alternately in one process
(the format of tools/bench_inference.py --lengths), with the largest difference to each cloud run alone.

One JSON line per case in the format of profiles/inference_forward.json: ms per forward and clouds/s of both paths (median over the
windows), each path's min / max, library launches per forward, the Predictor's algorithmic FLOPs and compulsory HBM bytes per
forward (from the shapes), the max-abs difference of the two paths' outputs, and `faster`: the acceptance condition
median(eval) - median(predictor) > spread(eval) + spread(predictor)."""
import argparse
import datetime
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_inference import launches, window  # noqa: E402  (also puts the package on sys.path)

import torch  # noqa: E402


def algorithmic(model, B, N):
    """FLOPs (2 per multiply-add) and compulsory HBM bytes of one Predictor forward, from the shapes: the input read once per trunk,
    every folded weight and transform read once, the pooled features and head activations written and read once."""
    enc = model.encoder
    ft = enc.feature_transform
    D = enc.conv1.weight.shape[1]
    chains = [[D, 64, 128, 1024]] + ([[D, 64, 64, 128, 1024]] if ft else []) + [[D, 64] + ([64] if ft else []) + [128, 1024]]
    flops = nbytes = 0
    for ch in chains:
        flops += sum(2 * B * N * a * b for a, b in zip(ch, ch[1:]))
        nbytes += 4 * (B * N * D + sum(a * b + b for a, b in zip(ch, ch[1:])) + B * 1024)
    heads = [(1024, 512), (512, 256), (256, 9)] + ([(1024, 512), (512, 256), (256, 4096)] if ft else []) + [(1024, 512), (512, 256), (256, 3)]
    for k, n in heads:
        flops += 2 * B * k * n
        nbytes += 4 * (k * n + n + B * (k + n))
    return flops, nbytes


def make(feature_transform):
    from models.pointnet import PointNet
    torch.manual_seed(0)
    model = PointNet(feature_transform).cuda().eval()
    with torch.no_grad():   # statistics off their initial values, as after training
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return model


def case(feature_transform, B, N, windows, seconds):
    from pnpp_hip import Predictor
    model = make(feature_transform)
    pred = Predictor(model)
    x = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(1234)).cuda()

    def run_eval():
        with torch.no_grad():
            return model(x)

    def run_pred():
        return pred(x)

    diff = float((run_eval() - run_pred()).abs().max())
    for _ in range(5):
        run_eval(), run_pred()
    torch.cuda.synchronize()
    n_eval, n_pred = launches(run_eval), launches(run_pred)
    t_eval, t_pred, r_eval, r_pred = [], [], 8, 8
    for _ in range(windows):   # alternately: drift of the clocks hits both paths alike
        ms, r_eval = window(run_eval, seconds, r_eval)
        t_eval.append(ms)
        ms, r_pred = window(run_pred, seconds, r_pred)
        t_pred.append(ms)
    flops, nbytes = algorithmic(model, B, N)
    me, mp = statistics.median(t_eval), statistics.median(t_pred)
    se, sp = max(t_eval) - min(t_eval), max(t_pred) - min(t_pred)
    return {
        "model": f"PointNet(feature_transform={feature_transform})", "B": B, "N": N, "date": datetime.date.today().isoformat(),
        "device": torch.cuda.get_device_name(0), "windows": windows, "window_s": seconds,
        "eval_ms": round(me, 4), "eval_ms_min": round(min(t_eval), 4), "eval_ms_max": round(max(t_eval), 4),
        "eval_clouds_per_s": round(1e3 * B / me, 1), "eval_launches": n_eval,
        "predictor_ms": round(mp, 4), "predictor_ms_min": round(min(t_pred), 4), "predictor_ms_max": round(max(t_pred), 4),
        "predictor_clouds_per_s": round(1e3 * B / mp, 1), "predictor_launches": n_pred,
        "predictor_flops": flops, "predictor_hbm_bytes": nbytes, "plan": pred.plan,
        "max_abs_diff": diff, "speedup": round(me / mp, 3), "faster": bool(me - mp > se + sp),
    }


def ragged_case(B, N, windows, seconds):
    import benchline
    from bench_inference import ragged_bank_batch
    from bench_pt_inference import alternate, ragged_record
    from pnpp_hip import Predictor
    pred = Predictor(make(True))
    xyz, dev_lengths, lengths, full = ragged_bank_batch(B, N)
    runs = {"ragged": lambda: pred(xyz, lengths=dev_lengths), "resampled": lambda: pred(full)}
    alone = torch.cat([pred(xyz[b:b + 1, :int(n)].contiguous()) for b, n in enumerate(lengths)])
    diff = float((runs["ragged"]() - alone).abs().max())
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    rec = {"model": "PointNet(feature_transform=True)", "B": B, "N": N, "date": datetime.date.today().isoformat(),
           "device": torch.cuda.get_device_name(0), "windows": windows, "window_s": seconds,
           "workload": "Predictor(PointNet) forward, ragged batch (DeviceCloudBank.padded) against every cloud resampled to N rows "
                       "(DeviceCloudBank.sample)",
           "plan": pred.last_plan, "launches": {k: launches(fn) for k, fn in runs.items()}, "max_abs_diff_to_each_cloud_alone": diff,
           # device time of the library's kernels alone (instrumented, serialised launches): what the early-leaving tiles save
           "kernel_ms_per_forward": {k: round(sum(r[2] for r in benchline.profiled_rows(fn, 5)) / 5, 4) for k, fn in runs.items()}}
    return ragged_record(rec, alternate(runs, windows, seconds, 8), lengths, N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per window")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (overwritten)")
    ap.add_argument("--trace-only", type=int, default=0, help="run this many Predictor forwards (PointNet(True), B=32, N=1024) and exit")
    ap.add_argument("--lengths", action="store_true",
                    help="a ragged batch (seeded lengths, uniform on [N/4, N], from a DeviceCloudBank) against every cloud resampled to N "
                         "rows, at 32 x 1024; --out is appended to")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pointnet_inference needs an AMD GPU"
    if args.lengths:
        line = json.dumps(ragged_case(32, 1024, args.windows, args.window))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        return
    if args.trace_only:
        from pnpp_hip import Predictor
        pred = Predictor(make(True))
        x = torch.randn(32, 1024, 3, generator=torch.Generator().manual_seed(1234)).cuda()
        for _ in range(args.trace_only):
            pred(x)
        torch.cuda.synchronize()
        return
    lines = []
    for ft, B, N in ((True, 32, 1024), (False, 32, 1024), (True, 256, 1024)):
        lines.append(json.dumps(case(ft, B, N, args.windows, args.window)))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
