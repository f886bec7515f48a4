#!/usr/bin/env python
"""Forward-only throughput: model.eval() under no_grad against pnpp_hip.inference.Predictor, timed alternately in one process.

    python tools/bench_inference.py                    # PointNetPPVonMises B=32 N=1024, then PointNetPP8Dir B=256 N=2048
    python tools/bench_inference.py --out profiles/inference_forward.json
    python tools/bench_inference.py --trace-only 20    # ~20 Predictor forwards and nothing else (run it under a kernel trace)

One JSON line per case: clouds/s and ms per forward of both paths (median over the windows), each path's min-max spread, library
launches per forward (kernels the library itself launches; torch's own copies and fills are not counted), the Predictor's algorithmic FLOPs and compulsory HBM bytes per forward (from the shapes), the max-abs
difference of the two paths' outputs, and `faster`: the acceptance condition median(eval) - median(predictor) > spread(eval) +
spread(predictor).  Windows are timed with device events closed by a synchronise; each is at least --window seconds long.
"""
import argparse
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


def clouds(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, N, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 0.6, 0.3])).cuda()


def algorithmic(model, B, N):
    """FLOPs (2 per multiply-add) and compulsory HBM bytes of one Predictor forward, from the shapes: every input, index, folded
    weight and output read or written once; the M x C tiles never leave the chip."""
    flops = nbytes = 0
    n_in = N
    for sa in (model.sa1, model.sa2, model.sa3):
        ch = [c.weight.shape[0] for c in sa.convs]
        cin = sa.convs[0].weight.shape[1]
        S, K = (1, n_in) if sa.group_all else (sa.npoint, sa.nsample)
        M = B * S * K
        widths = [cin] + ch
        flops += sum(2 * M * widths[i] * widths[i + 1] for i in range(3))
        weights = sum(widths[i] * widths[i + 1] + widths[i + 1] for i in range(3))
        # source rows (coordinates + features), neighbour and centre indices, weights, pooled output and new_xyz
        nbytes += 4 * (B * n_in * cin + (0 if sa.group_all else M + B * S) + weights + B * S * ch[-1] + B * S * 3)
        n_in = S
    for fc in (model.fc1, model.fc2):
        flops += 2 * B * fc.weight.numel()
        nbytes += 4 * (fc.weight.numel() + fc.bias.numel() + B * sum(fc.weight.shape))
    return flops, nbytes


def launches(fn):
    from pnpp_hip import _lib
    lib = _lib.lib()
    fn()
    torch.cuda.synchronize()
    lib.pnpp_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    buf = (b"\0" * (1 << 16))
    import ctypes
    cbuf = ctypes.create_string_buffer(buf, len(buf))
    lib.pnpp_profile_report(cbuf, len(buf))
    lib.pnpp_profile_enable(0)
    return sum(int(line.split("\t")[1]) for line in cbuf.value.decode().splitlines() if line.count("\t") >= 2)


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


def case(cls, B, N, windows, seconds):
    from pnpp_hip.inference import Predictor
    torch.manual_seed(0)
    model = cls(sampler="device").cuda().eval()
    with torch.no_grad():   # statistics off their initial values, as after training
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    pred = Predictor(model)
    xyz = clouds(B, N, 1234)

    def run_eval():
        with torch.no_grad():
            return model(xyz)

    def run_pred():
        return pred(xyz)

    from pnpp_hip import ops
    with torch.no_grad():   # both paths on the same centres for the output difference
        c1 = ops.sample_random(1, 0, B, N, model.sa1.npoint, xyz.device)
        c2 = ops.sample_random(1, 1, B, model.sa1.npoint, model.sa2.npoint, xyz.device)
        oe, op = model(xyz, centres=(c1, c2)), pred(xyz, centres=(c1, c2))
    as_t = lambda o: o if isinstance(o, (tuple, list)) else (o,)
    diff = max(float((a - b).abs().max()) for a, b in zip(as_t(oe), as_t(op)))
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
        "model": cls.__name__, "B": B, "N": N, "sampler": "device", "date": datetime.date.today().isoformat(),
        "device": torch.cuda.get_device_name(0), "windows": windows, "window_s": seconds,
        "eval_ms": round(me, 4), "eval_ms_min": round(min(t_eval), 4), "eval_ms_max": round(max(t_eval), 4),
        "eval_clouds_per_s": round(1e3 * B / me, 1), "eval_launches": n_eval,
        "predictor_ms": round(mp, 4), "predictor_ms_min": round(min(t_pred), 4), "predictor_ms_max": round(max(t_pred), 4),
        "predictor_clouds_per_s": round(1e3 * B / mp, 1), "predictor_launches": n_pred,
        "predictor_flops": flops, "predictor_hbm_bytes": nbytes, "plan": pred.plan,
        "max_abs_diff": diff, "speedup": round(me / mp, 3), "faster": bool(me - mp > se + sp),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per window")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (overwritten)")
    ap.add_argument("--trace-only", type=int, default=0, help="run this many Predictor forwards (B=32, N=1024) and exit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_inference needs an AMD GPU"
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    from models.pointnet_pp_8dir import PointNetPP8Dir
    if args.trace_only:
        from pnpp_hip.inference import Predictor
        torch.manual_seed(0)
        pred = Predictor(PointNetPPVonMises(sampler="device").cuda().eval())
        xyz = clouds(32, 1024, 1234)
        for _ in range(args.trace_only):
            pred(xyz)
        torch.cuda.synchronize()
        return
    lines = []
    for cls, B, N in ((PointNetPPVonMises, 32, 1024), (PointNetPP8Dir, 256, 2048)):
        lines.append(json.dumps(case(cls, B, N, args.windows, args.window)))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
