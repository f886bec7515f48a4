#!/usr/bin/env python
"""Forward-only throughput of the point transformer: model.eval() under no_grad against pnpp_hip.Predictor, timed alternately in one
process (window() / launches() of tools/bench_inference.py).

    python tools/bench_pt_inference.py                  # PointTransformer() at 8 x 4096 (the configs[4] per-GPU shard) and 32 x 1024
    python tools/bench_pt_inference.py --out profiles/pt_inference_forward.json
    python tools/bench_pt_inference.py --trace-only 10  # ~10 forwards of EACH path at 8 x 4096 and nothing else (for a kernel trace)

One JSON line per shape in the format of profiles/pointnet_inference_forward.json: ms per forward and clouds/s of both paths (median
over the windows), each path's min / max, library launches per forward, the Predictor's algorithmic FLOPs and compulsory HBM bytes per
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


def algorithmic(model, B, n_pts):
    """FLOPs (2 per multiply-add) and compulsory HBM bytes of one Predictor forward, from the shapes: the dense products and the
    attention's two products per head; the input, every weight, and per layer x, qkv and the attention output written and read once
    (the hidden activation never leaves the chip)."""
    E, K = model.input_proj.out_features, model.input_proj.in_features
    depth = len(model.transformer.layers)
    F = model.transformer.layers[0].linear1.out_features
    N = (n_pts + 127) // 128 * 128
    M = B * N
    per_layer = 2 * M * E * (3 * E + E + 2 * F) + 4 * B * N * N * E
    flops = 2 * M * K * E + depth * per_layer + 2 * B * E * 3
    weights = 4 * (K * E + E) + depth * (6 * (4 * E * E + 2 * E * F) + 4 * (3 * E + E + F + E + 4 * E))
    nbytes = 4 * B * n_pts * K + weights + depth * 4 * M * (2 * E + 2 * 3 * E + 2 * E + E) + 4 * B * 3
    return flops, nbytes


def make():
    from models.point_transformer import PointTransformer
    torch.manual_seed(0)
    return PointTransformer().cuda().eval()


def cloud(B, N):
    return torch.randn(B, N, 3, generator=torch.Generator().manual_seed(1234)).cuda()


def case(B, N, windows, seconds):
    from pnpp_hip import Predictor
    model = make()
    pred = Predictor(model)
    x = cloud(B, N)

    def run_eval():
        with torch.no_grad():
            return model(x)

    def run_pred():
        return pred(x)

    diff = float((run_eval() - run_pred()).abs().max())
    for _ in range(3):
        run_eval(), run_pred()
    torch.cuda.synchronize()
    n_eval, n_pred = launches(run_eval), launches(run_pred)
    t_eval, t_pred, r_eval, r_pred = [], [], 4, 4
    for _ in range(windows):   # alternately: drift of the clocks hits both paths alike
        ms, r_eval = window(run_eval, seconds, r_eval)
        t_eval.append(ms)
        ms, r_pred = window(run_pred, seconds, r_pred)
        t_pred.append(ms)
    flops, nbytes = algorithmic(model, B, N)
    me, mp = statistics.median(t_eval), statistics.median(t_pred)
    se, sp = max(t_eval) - min(t_eval), max(t_pred) - min(t_pred)
    return {
        "model": "PointTransformer()", "B": B, "N": N, "date": datetime.date.today().isoformat(),
        "device": torch.cuda.get_device_name(0), "windows": windows, "window_s": seconds,
        "eval_ms": round(me, 4), "eval_ms_min": round(min(t_eval), 4), "eval_ms_max": round(max(t_eval), 4),
        "eval_clouds_per_s": round(1e3 * B / me, 1), "eval_launches": n_eval,
        "predictor_ms": round(mp, 4), "predictor_ms_min": round(min(t_pred), 4), "predictor_ms_max": round(max(t_pred), 4),
        "predictor_clouds_per_s": round(1e3 * B / mp, 1), "predictor_launches": n_pred,
        "predictor_flops": flops, "predictor_hbm_bytes": nbytes, "plan": pred.last_plan,
        "max_abs_diff": diff, "speedup": round(me / mp, 3), "faster": bool(me - mp > se + sp),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per window")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (overwritten)")
    ap.add_argument("--trace-only", type=int, default=0, help="run this many forwards of each path at 8 x 4096 and exit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pt_inference needs an AMD GPU"
    if args.trace_only:
        from pnpp_hip import Predictor
        model = make()
        pred = Predictor(model)
        x = cloud(8, 4096)
        for _ in range(args.trace_only):
            pred(x)
            with torch.no_grad():
                model(x)
        torch.cuda.synchronize()
        return
    lines = []
    for B, N in ((8, 4096), (32, 1024)):
        lines.append(json.dumps(case(B, N, args.windows, args.window)))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
