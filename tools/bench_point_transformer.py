#!/usr/bin/env python3
"""Timing of one training step of BASELINE config 5 (models/point_transformer.py, N=4096, 8 clouds per GPU = batch 64
over 8 GPUs) on one MI355X: forward + MSE harness loss + backward + fused Adam (--dropout sets the encoder layers' dropout probability).  Not the driver's bench line (that is bench.py / configs[1]); prints one JSON line
in bench.py's format (tools/benchline.py: `roofline` for its costliest kernel) plus the per-kernel time table and the attention kernels' TFLOP/s.

--attention float32|split chooses the form of the training attention (PointTransformer.set_attention).  --attention both runs the two
forms alternately in one process, in windows (as tools/bench_pt_inference.py), and prints one JSON line with, per form: ms per step (median
of the windows), the spread of the windows, the three attention kernels' per-launch times and TFLOP/s from one profiled step, and final_loss;
--out appends that line to a file (profiles/pt_attention_training.json holds the four lines of 8 x 4096 and 32 x 1024 at dropout 0 and 0.1).

--lengths times the step on a RAGGED batch (seeded per-cloud lengths, uniform on [N/4, N], model(xyz, lengths)) against the status quo for
the same clouds (every cloud resampled to N rows with replacement, no lengths), at 8 x 4096 and 32 x 1024 in the form --attention names,
the two paths alternately in the same windows; one JSON line per shape (tools/bench_pt_inference.py says what the fields are), appended
to --out (profiles/pt_ragged.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402


FORMS = ("float32", "split")


def attention_rows(rows, batch, points, heads=4, dh=16):
    """the attention kernels among the profiled rows: per-launch microseconds and TFLOP/s (2 flops per multiply-add; the forward forms two
    products, dQ three, dK/dV four)"""
    fwd = 4.0 * batch * heads * points * points * dh
    out = []
    for tag, cnt, ms in rows:
        for head, f in (("attention_fwd", 1.0), ("attention_bwd_dq", 1.5), ("attention_bwd_dkv", 2.0)):
            if tag.startswith(head):
                out.append({"kernel": tag, "launches": cnt, "us_per_launch": round(1e3 * ms / cnt, 1),
                            "tflops": round(f * fwd * cnt / (ms * 1e-3) / 1e12, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.0, help="dropout probability of the encoder layers (reference default 0.1)")
    ap.add_argument("--attention", choices=FORMS + ("both",), default="float32",
                    help="the form of the training attention (PointTransformer.set_attention); both: the two forms alternately, in windows")
    ap.add_argument("--windows", type=int, default=5, help="--attention both: windows per form")
    ap.add_argument("--window", type=float, default=0.5, help="--attention both: seconds of device time per window")
    ap.add_argument("--out", default=None, help="--attention both / --lengths: also append the JSON line to this file")
    ap.add_argument("--lengths", action="store_true",
                    help="a ragged batch (seeded lengths, uniform on [N/4, N]) against every cloud resampled to N rows, at 8 x 4096 and 32 x 1024")
    a = ap.parse_args()
    if a.lengths:
        for B, N in ((8, 4096), (32, 1024)):
            ragged(a, B, N)
        return
    from models.point_transformer import PointTransformer
    from pnpp_hip import _lib, ops, optim
    import benchline
    import synthetic
    xyz, _, _, fwd = synthetic.rotated_clouds(a.batch, a.points, seed=1234)
    xyz, tgt = xyz.cuda(), fwd.cuda()

    def make(form):
        torch.manual_seed(42)
        model = PointTransformer().cuda().train().set_dropout(a.dropout).set_attention(form)
        opt = optim.FlatAdam(model.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            loss = ops.mse_loss(model(xyz), tgt)
            loss.backward()
            opt.step()
            return loss
        return model, step

    if a.attention == "both":
        both(a, make)
        return
    model, step = make(a.attention)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    rows = benchline.profiled_rows(step, 1)
    H, dh, L = 4, 16, len(model.transformer.layers)
    att_flops_fwd = 4.0 * a.batch * H * a.points * a.points * dh          # QK^T and PV, 2 flops per MAC
    table = []
    for tag, cnt, ms in rows[:12]:
        e = {"kernel": tag, "launches": cnt, "ms": round(ms, 3)}
        if tag.startswith("attention_fwd"):
            e["tflops"] = round(att_flops_fwd * cnt / (ms * 1e-3) / 1e12, 1)
        if tag.startswith("attention_bwd_dq"):
            e["tflops"] = round(1.5 * att_flops_fwd * cnt / (ms * 1e-3) / 1e12, 1)   # S, dP, dQ
        if tag.startswith("attention_bwd_dkv"):
            e["tflops"] = round(2.0 * att_flops_fwd * cnt / (ms * 1e-3) / 1e12, 1)   # S, dP, dV, dK
        table.append(e)
    print(json.dumps(benchline.line(f"configs[4]: models/point_transformer.py N={a.points} batch={a.batch}/GPU, fwd+MSE+bwd+Adam, "
                                    f"dropout p={a.dropout}, attention={a.attention}", a.batch, dt, a.steps, a.warmup, rows, 1, layers=L,
                                    final_loss=float(loss.detach()), top_kernels=table)))


def ragged(a, B, N):
    """One training step on a ragged batch against the same clouds resampled to N rows: one model and optimiser each from the same seed,
    timed alternately in windows."""
    from models.point_transformer import PointTransformer
    from pnpp_hip import ops, optim
    from bench_pt_inference import alternate, ragged_batch, ragged_record
    form = "float32" if a.attention == "both" else a.attention
    x, lengths, full = ragged_batch(B, N)
    dev_lengths = lengths.to(torch.int32).cuda()
    tgt = torch.randn(B, 3, generator=torch.Generator().manual_seed(7)).cuda()
    loss = {}

    def make(name, xyz, lens):
        torch.manual_seed(42)
        model = PointTransformer().cuda().train().set_dropout(a.dropout).set_attention(form)
        opt = optim.FlatAdam(model.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            loss[name] = ops.mse_loss(model(xyz, lens), tgt)
            loss[name].backward()
            opt.step()
        return step

    runs = {"ragged": make("ragged", x, dev_lengths), "resampled": make("resampled", full, None)}
    for _ in range(a.warmup):
        for step in runs.values():
            step()
    torch.cuda.synchronize()
    res = alternate(runs, a.windows, a.window, 2)
    rec = {"workload": "models/point_transformer.py fwd+MSE+bwd+Adam, ragged batch against every cloud resampled to N rows", "B": B, "N": N,
           "dropout": a.dropout, "attention": form, "device": torch.cuda.get_device_name(0), "windows": a.windows, "window_s": a.window,
           "final_loss": {k: float(v.detach()) for k, v in loss.items()}}
    line = json.dumps(ragged_record(rec, res, lengths, N))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def both(a, make):
    """The two forms in one process: one model and optimiser each from the same seed, timed alternately in windows (drift of the clocks
    hits both alike), then one profiled step each for the attention kernels' per-launch times."""
    import statistics
    import benchline
    from bench_inference import window
    raw = {form: make(form)[1] for form in FORMS}
    loss, taken = {}, {form: 0 for form in FORMS}

    def counted(form):
        def step():
            taken[form] += 1
            loss[form] = raw[form]()
        return step

    steps = {form: counted(form) for form in FORMS}
    for _ in range(a.warmup):
        for step in steps.values():
            step()
    torch.cuda.synchronize()
    t, reps = {form: [] for form in FORMS}, {form: 2 for form in FORMS}
    for _ in range(a.windows):
        for form, step in steps.items():
            ms, reps[form] = window(step, a.window, reps[form])
            t[form].append(ms)
    torch.cuda.synchronize()
    med = {form: statistics.median(v) for form, v in t.items()}
    spread = {form: max(v) - min(v) for form, v in t.items()}
    rec = {"workload": f"models/point_transformer.py N={a.points} batch={a.batch}/GPU, fwd+MSE+bwd+Adam", "B": a.batch, "N": a.points,
           "dropout": a.dropout, "device": torch.cuda.get_device_name(0), "windows": a.windows, "window_s": a.window}
    for form, step in steps.items():   # final_loss: after steps_taken optimiser steps -- a window is timed, not counted, so the faster form has taken more
        rows = benchline.profiled_rows(step, 1)
        rec[form] = {"ms_per_step": round(med[form], 4), "ms_min": round(min(t[form]), 4), "ms_max": round(max(t[form]), 4),
                     "spread_ms": round(spread[form], 4), "steps_taken": taken[form], "final_loss": float(loss[form].detach()),
                     "kernel_ms_per_step": round(sum(r[2] for r in rows), 3), "attention_kernels": attention_rows(rows, a.batch, a.points)}
    rec["speedup"] = round(med["float32"] / med["split"], 4)
    # the rule DESIGN section 11 used for the Predictor's default: faster by more than the spread of the windows
    rec["split_faster"] = bool(med["float32"] - med["split"] > spread["float32"] + spread["split"])
    rec["float32_faster"] = bool(med["split"] - med["float32"] > spread["float32"] + spread["split"])
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
