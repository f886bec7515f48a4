#!/usr/bin/env python
"""Forward-only throughput: model.eval() under no_grad against pnpp_hip.inference.Predictor, timed alternately in one process.

    python tools/bench_inference.py                    # PointNetPPVonMises B=32 N=1024, then PointNetPP8Dir B=256 N=2048
    python tools/bench_inference.py --out profiles/inference_forward.json
    python tools/bench_inference.py --trace-only 20    # ~20 Predictor forwards and nothing else (run it under a kernel trace)

One JSON line per case: clouds/s and ms per forward of both paths (median over the windows), each path's min-max spread, library
launches per forward (kernels the library itself launches; torch's own copies and fills are not counted), the Predictor's algorithmic FLOPs and compulsory HBM bytes per forward (from the shapes), the max-abs
difference of the two paths' outputs, and `faster`: the acceptance condition median(eval) - median(predictor) > spread(eval) +
spread(predictor).  Windows are timed with device events closed by a synchronise; each is at least --window seconds long.

    python tools/bench_inference.py --lengths --out profiles/sa_ragged.json   # appends one line per path (Predictor, training step)

--lengths times a RAGGED batch of PointNetPPVonMises at 32 x 1024 -- DeviceCloudBank.padded(ids) of a bank whose clouds have seeded
lengths, uniform on [N/4, N] (the first cloud keeps N points, so the padded batch has N rows) -- against the status quo for the same
clouds: bank.sample(ids, N), every cloud resampled to N rows, run without lengths.  The two paths alternate in one process, in the same
windows (alternate() / ragged_record() of tools/bench_pt_inference.py, which says what the fields are).  Only the index kernels' work
shrinks with the lengths, so there is no speed target: `ragged_not_slower` is median(ragged) - median(resampled) <= spread(ragged) +
spread(resampled).
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


def ragged_bank_batch(B, N, seed=2048):
    """a bank of B clouds with seeded lengths, uniform on [N/4, N] (cloud 0 keeps N points) -> the ragged batch bank.padded(ids) =
    (xyz (B, N, 3), lengths (B,) int32, both on the device), the host lengths, and bank.sample(ids, N): every cloud resampled to N rows"""
    from dataloader_common import DeviceCloudBank
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(N // 4, N + 1, (B,), generator=g)
    lengths[0] = N
    box = torch.tensor([1.0, 0.6, 0.3])
    bank = DeviceCloudBank([((torch.rand(int(n), 3, generator=g) * 2 - 1) * box).numpy() for n in lengths], "cuda", seed=seed)
    ids = list(range(B))
    xyz, dev_lengths = bank.padded(ids)
    return xyz, dev_lengths, lengths, bank.sample(ids, N)


def ragged_cases(B, N, windows, seconds):
    """Predictor forward and one training step (forward, fused head + KL loss + backward) of PointNetPPVonMises(sampler='device'):
    the ragged batch against the resampled one"""
    from bench_pt_inference import alternate, ragged_record
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    torch.manual_seed(0)
    model = PointNetPPVonMises(sampler="device").cuda()
    xyz, dev_lengths, lengths, full = ragged_bank_batch(B, N)
    g = torch.Generator().manual_seed(7)
    mu_gt, kappa_gt = ((torch.rand(B, generator=g) * 2 - 1) * 3.14).cuda(), torch.full((B,), 8.0).cuda()
    base = {"model": "PointNetPPVonMises", "sampler": "device", "B": B, "N": N, "date": datetime.date.today().isoformat(),
            "device": torch.cuda.get_device_name(0), "windows": windows, "window_s": seconds}
    out = []

    def step(x, L):
        model.zero_grad(set_to_none=True)
        return ops.vm_head_kl_loss(model.features(x, lengths=L), mu_gt, kappa_gt).backward()

    model.train()
    runs = {"ragged": lambda: step(xyz, dev_lengths), "resampled": lambda: step(full, None)}
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    rec = dict(base, workload="PointNetPPVonMises forward + fused head / KL loss + backward, ragged batch (DeviceCloudBank.padded) against "
               "every cloud resampled to N rows (DeviceCloudBank.sample)", launches={k: launches(fn) for k, fn in runs.items()})
    out.append(ragged_record(rec, alternate(runs, windows, seconds, 8), lengths, N))

    model.eval()
    pred = Predictor(model)
    runs = {"ragged": lambda: pred(xyz, lengths=dev_lengths), "resampled": lambda: pred(full)}
    c1 = ops.sample_random(1, 0, B, N, model.sa1.npoint, xyz.device, lengths=dev_lengths)
    c2 = ops.sample_random(1, 1, B, model.sa1.npoint, model.sa2.npoint, xyz.device)
    both = pred(xyz, centres=(c1, c2), lengths=dev_lengths)
    alone = [pred(xyz[b:b + 1, :int(n)].contiguous(), centres=(c1[b:b + 1], c2[b:b + 1])) for b, n in enumerate(lengths)]
    diff = max(float((both[i] - torch.cat([a[i] for a in alone])).abs().max()) for i in range(len(both)))
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    rec = dict(base, workload="Predictor(PointNetPPVonMises) forward, ragged batch (DeviceCloudBank.padded) against every cloud resampled "
               "to N rows (DeviceCloudBank.sample)", plan=pred.last_plan, launches={k: launches(fn) for k, fn in runs.items()},
               max_abs_diff_to_each_cloud_alone=diff)
    out.append(ragged_record(rec, alternate(runs, windows, seconds, 8), lengths, N))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per window")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (overwritten)")
    ap.add_argument("--trace-only", type=int, default=0, help="run this many Predictor forwards (B=32, N=1024) and exit")
    ap.add_argument("--lengths", action="store_true",
                    help="a ragged batch (seeded lengths, uniform on [N/4, N], from a DeviceCloudBank) against every cloud resampled to N "
                         "rows, at 32 x 1024; --out is appended to")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_inference needs an AMD GPU"
    if args.lengths:
        for rec in ragged_cases(32, 1024, args.windows, args.window):
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        return
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
