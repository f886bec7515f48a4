#!/usr/bin/env python
"""Forward-only throughput of the point transformer: model.eval() under no_grad against pnpp_hip.Predictor with each of its two attention
forms ("split": pnpp_attention_infer, "float32": pnpp_attention_fwd), the three paths timed alternately in one process (window() /
launches() of tools/bench_inference.py).

    python tools/bench_pt_inference.py                  # PointTransformer() at 8 x 4096 (the configs[4] per-GPU shard) and 32 x 1024
    python tools/bench_pt_inference.py --out profiles/pt_attention_inference.json
    python tools/bench_pt_inference.py --trace-only 10  # ~10 forwards of EACH path at 8 x 4096 and nothing else (for a kernel trace)

--trace-only is what a `rocprofv3 --kernel-trace --stats -- python tools/bench_pt_inference.py --trace-only 10` run of its own traces:
the two attention kernels have different names (attention_infer_kernel, attention_fwd_kernel), so the per-launch times of both come
from the same run; its kernel_stats.csv is what profiles/pt_attention_kernel_stats.csv holds.

One JSON line per shape in the format of profiles/pointnet_inference_forward.json: ms per forward and clouds/s of the paths (median
over the windows; `predictor_*` is the Predictor as it is built by default, `attention` its form, `predictor_<other form>_*` the other),
each path's min / max, library launches per forward, the Predictor's algorithmic FLOPs and compulsory HBM bytes per forward (from the
shapes), the max-abs difference of the paths' outputs, `faster`: the acceptance condition median(eval) - median(predictor) >
spread(eval) + spread(predictor), `attention_speedup` / `attention_faster`: float32 over split and the same condition between the two attention forms, and
`attention_err_split` / `attention_err_float32`: max |attend(qkv_0) - float64| over cloud 0, float64 softmax attention on the float32
qkv of layer 0.

    python tools/bench_pt_inference.py --lengths --out profiles/pt_ragged.json   # appends one line per shape

--lengths times a RAGGED batch -- seeded per-cloud lengths, uniform on [N/4, N], Predictor(model)(xyz, lengths) -- against the status quo
for the same clouds: every cloud resampled to N rows with replacement (what dataloader_common.sample_pts does for a short cloud) and run
without lengths.  The two paths alternate in one process, in the same windows.  `ragged_not_slower` is the condition that follows from
the code (the ragged batch does a subset of the full batch's work): median(ragged) - median(resampled) <= spread(ragged) + spread(resampled)."""
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


def ragged_batch(B, N, seed=2048):
    """(xyz (B, N, 3) whose cloud b is its first lengths[b] rows, lengths (B,) int64 on the host, seeded and uniform on [N/4, N], and the
    status quo for the same clouds: every cloud resampled to N rows with replacement), all but the lengths on the GPU"""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(N // 4, N + 1, (B,), generator=g)
    x = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(1234))
    full = torch.stack([x[b, torch.randint(0, int(n), (N,), generator=g)] for b, n in enumerate(lengths)])
    return x.cuda(), lengths, full.cuda()


def alternate(runs, windows, seconds, reps0):
    """the paths timed alternately in windows: {path: {"ms", "ms_min", "ms_max", "spread_ms"}} (median, extremes and spread of the windows)"""
    t, reps = {k: [] for k in runs}, {k: reps0 for k in runs}
    for _ in range(windows):   # alternately: drift of the clocks hits every path alike
        for k, fn in runs.items():
            ms, reps[k] = window(fn, seconds, reps[k])
            t[k].append(ms)
    return {k: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "spread_ms": round(max(v) - min(v), 4)}
            for k, v in t.items()}


def ragged_record(rec, res, lengths, N):
    """the fields both --lengths tools report"""
    rec.update({"lengths": [int(n) for n in lengths], "mean_length_over_N": round(float(lengths.double().mean()) / N, 4), **res})
    rec["ragged_over_resampled"] = round(res["ragged"]["ms"] / res["resampled"]["ms"], 4)
    rec["ragged_not_slower"] = bool(res["ragged"]["ms"] - res["resampled"]["ms"] <= res["ragged"]["spread_ms"] + res["resampled"]["spread_ms"])
    return rec


def ragged_case(B, N, windows, seconds):
    from pnpp_hip import Predictor
    model = make()
    pred = Predictor(model)
    x, lengths, full = ragged_batch(B, N)
    dev_lengths = lengths.to(torch.int32).cuda()   # on the device already: used as it is, no synchronisation per call
    runs = {"ragged": lambda: pred(x, dev_lengths), "resampled": lambda: pred(full)}
    alone = torch.cat([pred(x[b:b + 1, :int(n)].contiguous()) for b, n in enumerate(lengths)])
    diff = float((runs["ragged"]() - alone).abs().max())
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    res = alternate(runs, windows, seconds, 4)
    rec = {"workload": "Predictor(PointTransformer()) forward, ragged batch against every cloud resampled to N rows", "B": B, "N": N,
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "windows": windows, "window_s": seconds,
           "attention": pred.last_attention, "plan": pred.last_plan, "max_abs_diff_to_each_cloud_alone": diff}
    return ragged_record(rec, res, lengths, N)


def attention_errors(preds, x):
    """max |attend(qkv_0) - float64| over cloud 0 for each form: float64 softmax attention on the float32 qkv of layer 0"""
    E = preds["split"].model.input_proj.out_features
    heads = preds["split"].model.transformer.layers[0].self_attn.num_heads
    n = x.shape[1]
    qkv = preds["split"].head(x)[1][:1, :n].clone()
    q, k, v = (t.reshape(n, heads, E // heads).transpose(0, 1) for t in qkv[0].cpu().double().split(E, dim=-1))
    ref = (torch.softmax((q * (E // heads) ** -0.5) @ k.transpose(-1, -2), dim=-1) @ v).transpose(0, 1).reshape(n, E)
    return {form: float((p.attend(qkv)[0, :n].cpu().double() - ref).abs().max()) for form, p in preds.items()}


def case(B, N, windows, seconds):
    from pnpp_hip import Predictor
    model = make()
    default = Predictor(model).attention   # the form Predictor(model) runs: `predictor_*` below are that form's figures
    preds = {"split": Predictor(model, attention="split"), "float32": Predictor(model, attention="float32")}
    x = cloud(B, N)

    def run_eval():
        with torch.no_grad():
            return model(x)

    runs = {"eval": run_eval, "split": lambda: preds["split"](x), "float32": lambda: preds["float32"](x)}
    diff = {form: float((run_eval() - runs[form]()).abs().max()) for form in preds}
    errs = attention_errors(preds, x)
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    n = {k: launches(fn) for k, fn in runs.items()}
    t, reps = {k: [] for k in runs}, {k: 4 for k in runs}
    for _ in range(windows):   # alternately: drift of the clocks hits every path alike
        for k, fn in runs.items():
            ms, reps[k] = window(fn, seconds, reps[k])
            t[k].append(ms)
    flops, nbytes = algorithmic(model, B, N)
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: max(v) - min(v) for k, v in t.items()}
    me, mp, other = med["eval"], med[default], "float32" if default == "split" else "split"
    return {
        "model": "PointTransformer()", "B": B, "N": N, "date": datetime.date.today().isoformat(),
        "device": torch.cuda.get_device_name(0), "windows": windows, "window_s": seconds,
        "eval_ms": round(me, 4), "eval_ms_min": round(min(t["eval"]), 4), "eval_ms_max": round(max(t["eval"]), 4),
        "eval_clouds_per_s": round(1e3 * B / me, 1), "eval_launches": n["eval"],
        "attention": default,
        "predictor_ms": round(mp, 4), "predictor_ms_min": round(min(t[default]), 4), "predictor_ms_max": round(max(t[default]), 4),
        "predictor_clouds_per_s": round(1e3 * B / mp, 1), "predictor_launches": n[default],
        "predictor_flops": flops, "predictor_hbm_bytes": nbytes, "plan": preds[default].last_plan,
        "max_abs_diff": diff[default], "speedup": round(me / mp, 3), "faster": bool(me - mp > spread["eval"] + spread[default]),
        f"predictor_{other}_ms": round(med[other], 4), f"predictor_{other}_ms_min": round(min(t[other]), 4),
        f"predictor_{other}_ms_max": round(max(t[other]), 4), f"predictor_{other}_launches": n[other], f"max_abs_diff_{other}": diff[other],
        "attention_speedup": round(med["float32"] / med["split"], 3),
        "attention_faster": bool(med["float32"] - med["split"] > spread["float32"] + spread["split"]),
        "attention_err_split": errs["split"], "attention_err_float32": errs["float32"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per window")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (overwritten)")
    ap.add_argument("--trace-only", type=int, default=0, help="run this many forwards of each path at 8 x 4096 and exit")
    ap.add_argument("--lengths", action="store_true",
                    help="a ragged batch (seeded lengths, uniform on [N/4, N]) against every cloud resampled to N rows; --out is appended to")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pt_inference needs an AMD GPU"
    if args.lengths:
        for B, N in ((8, 4096), (32, 1024)):
            line = json.dumps(ragged_case(B, N, args.windows, args.window))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        return
    if args.trace_only:
        from pnpp_hip import Predictor
        model = make()
        pred, pred32 = Predictor(model, attention="split"), Predictor(model, attention="float32")
        x = cloud(8, 4096)
        for _ in range(args.trace_only):
            pred(x)
            pred32(x)
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
