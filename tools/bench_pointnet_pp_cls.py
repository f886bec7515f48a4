#!/usr/bin/env python
"""PointNetPlusPlusCls (models/pointnet_pp_cls.py) at 32 x 1024 x 6, the reference's level sizes:

    python tools/bench_pointnet_pp_cls.py --out profiles/pointnet_pp_cls.json

  - a training step (forward, nll loss, backward, torch.optim.Adam step): clouds/s and library launches,
  - Predictor against model.eval() under no_grad, timed alternately in one process (tools/bench_inference.py's windows),
  - per level, the fused launch (pnpp_sa_infer on given centres and neighbour lists) against the eval path's level on the same
    indices, and the farthest-point sampling and radius query in front of it on their own: FPS is serial per cloud, its share of the
    Predictor's forward is recorded.
One JSON document; `predictor_not_slower` is median(predictor) - median(eval) <= spread(eval) + spread(predictor).

    python tools/bench_pointnet_pp_cls.py --lengths --out profiles/sa_ragged.json   # appends one line per path

--lengths times a RAGGED batch (tools/bench_inference.py's ragged_bank_batch: DeviceCloudBank.padded of clouds with seeded lengths,
uniform on [N/4, N], random normals beside them) against the same clouds resampled to N rows and run without lengths -- a training
step and the Predictor's forward, the two paths alternating in the same windows (fields: tools/bench_pt_inference.py)."""
import argparse
import ctypes as C
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

from bench_inference import launches, window  # noqa: E402


def timed(fns, windows, seconds):
    """fns: {name: callable}, timed alternately -> {name: (median ms, min, max)}"""
    ts, reps = {k: [] for k in fns}, {k: 8 for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            ms, reps[k] = window(fn, seconds, reps[k])
            ts[k].append(ms)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def ragged_cases(B, N, windows, seconds):
    from bench_inference import ragged_bank_batch
    from bench_pt_inference import alternate, ragged_record
    from models import PointNetPlusPlusCls
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    torch.manual_seed(0)
    model = PointNetPlusPlusCls().cuda()
    xyz, dev_lengths, lengths, full = ragged_bank_batch(B, N)
    g = torch.Generator().manual_seed(1234)
    normals = torch.rand(B, N, 3, generator=g).cuda()
    x, x_full = (torch.cat([t, normals], -1).transpose(1, 2).contiguous() for t in (xyz, full))     # (B, 6, N)
    target = torch.randint(0, 40, (B,), generator=g).cuda()
    # the first indices injected (below every length): neither path draws on the host or reads the lengths back
    start = (torch.randint(0, N // 4, (B,), generator=g).cuda(), torch.randint(0, model.sa1.npoint, (B,), generator=g).cuda())
    base = {"model": "PointNetPlusPlusCls", "B": B, "N": N, "C": 6, "date": datetime.date.today().isoformat(),
            "device": torch.cuda.get_device_name(0), "windows": windows, "window_s": seconds}
    out = []
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)

    def step(inp, L):
        opt.zero_grad(set_to_none=True)
        ops.nll_loss(model(inp, start=start, lengths=L), target, check=False).backward()
        opt.step()

    model.train()
    runs = {"ragged": lambda: step(x, dev_lengths), "resampled": lambda: step(x_full, None)}
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    rec = dict(base, workload="PointNetPlusPlusCls forward + nll loss + backward + Adam, ragged batch (DeviceCloudBank.padded) against every "
               "cloud resampled to N rows (DeviceCloudBank.sample)", launches={k: launches(fn) for k, fn in runs.items()})
    out.append(ragged_record(rec, alternate(runs, windows, seconds, 8), lengths, N))

    model.eval()
    pred = Predictor(model)
    runs = {"ragged": lambda: pred(x, start=start, lengths=dev_lengths), "resampled": lambda: pred(x_full, start=start)}
    both = pred(x, start=start, lengths=dev_lengths)
    # each cloud alone, where the level takes it alone (a level refuses npoint > N; inside a padded batch a shorter cloud is legal)
    whole = [b for b, n in enumerate(lengths) if int(n) >= model.sa1.npoint]
    alone = torch.cat([pred(x[b:b + 1, :, :int(lengths[b])].contiguous(), start=(start[0][b:b + 1], start[1][b:b + 1])) for b in whole])
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    rec = dict(base, workload="Predictor(PointNetPlusPlusCls) forward, ragged batch (DeviceCloudBank.padded) against every cloud resampled to N "
               "rows (DeviceCloudBank.sample)", plan=pred.last_plan, launches={k: launches(fn) for k, fn in runs.items()},
               max_abs_diff_to_each_cloud_alone=float((both[whole] - alone).abs().max()), clouds_compared_alone=len(whole))
    out.append(ragged_record(rec, alternate(runs, windows, seconds, 8), lengths, N))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--lengths", action="store_true",
                    help="a ragged batch (seeded lengths, uniform on [N/4, N], from a DeviceCloudBank) against every cloud resampled to N "
                         "rows; --out is appended to")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pointnet_pp_cls needs an AMD GPU"
    if args.lengths:
        for rec in ragged_cases(args.B, args.N, args.windows, args.window):
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        return
    from models import PointNetPlusPlusCls
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    B, N = args.B, args.N
    torch.manual_seed(0)
    model = PointNetPlusPlusCls().cuda()
    with torch.no_grad():   # statistics off their initial values, as after training
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(B, 6, N, generator=g).cuda()
    target = torch.randint(0, 40, (B,), generator=g).cuda()
    res = {"model": "PointNetPlusPlusCls", "B": B, "N": N, "C": 6, "date": datetime.date.today().isoformat(),
           "device": torch.cuda.get_device_name(0), "windows": args.windows, "window_s": args.window}

    # training step
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        ops.nll_loss(model(x), target, check=False).backward()
        opt.step()

    model.train()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    res["train_launches"] = launches(step)
    med, lo, hi = timed({"train": step}, args.windows, args.window)["train"]
    res.update(train_ms=round(med, 4), train_ms_min=round(lo, 4), train_ms_max=round(hi, 4), train_clouds_per_s=round(1e3 * B / med, 1))

    # Predictor against model.eval()
    model.eval()
    pred = Predictor(model)

    def run_eval():
        with torch.no_grad():
            return model(x)

    def run_pred():
        return pred(x)

    start = (torch.randint(0, N, (B,)), torch.randint(0, model.sa1.npoint, (B,)))
    with torch.no_grad():
        res["max_abs_diff"] = float((model(x, start=start) - pred(x, start=start)).abs().max())
    for _ in range(3):
        run_eval(), run_pred()
    torch.cuda.synchronize()
    res["eval_launches"], res["predictor_launches"] = launches(run_eval), launches(run_pred)
    t = timed({"eval": run_eval, "predictor": run_pred}, args.windows, args.window)
    for k, (med, lo, hi) in t.items():
        res.update({f"{k}_ms": round(med, 4), f"{k}_ms_min": round(lo, 4), f"{k}_ms_max": round(hi, 4),
                    f"{k}_clouds_per_s": round(1e3 * B / med, 1)})
    (me, le, he), (mp, lp, hp) = t["eval"], t["predictor"]
    res.update(plan=pred.plan, last_plan=pred.last_plan, speedup=round(me / mp, 3),
               predictor_not_slower=bool(mp - me <= (he - le) + (hp - lp)))

    # per level: sampling, grouping, the fused launch, the eval path's level on the same indices
    levels = {}
    with torch.no_grad():
        xyz, pts = model.split_input(x)
        for i, sa in enumerate((model.sa1, model.sa2, model.sa3)):
            name = f"sa{i + 1}"
            fns = {}
            if sa.group_all:
                centre = nbr = None
                d = pred._takes(i, B, xyz.shape[1])
                K = None
            else:
                s = start[i].cuda()
                centre = sa._centres(xyz, s)
                new_xyz = ops.index_points(xyz, centre)
                nbr = ops.ball_query(sa.radius, sa.nsample, xyz, new_xyz)
                d = pred._takes(i, B, xyz.shape[1])
                K = sa.nsample
                fns["fps"] = lambda xyz=xyz, sa=sa, s=s: sa._centres(xyz, s)
                fns["ball_query"] = lambda xyz=xyz, sa=sa, new_xyz=new_xyz: ops.ball_query(sa.radius, sa.nsample, xyz, new_xyz)
            fns["fused"] = lambda i=i, d=d, xyz=xyz, pts=pts, centre=centre, nbr=nbr: pred._fused(i, d, xyz, pts, centre, nbr)
            fns["eval_path"] = lambda xyz=xyz, pts=pts, centre=centre, nbr=nbr, sa=sa, K=K: ops.set_abstraction(
                xyz, pts, centre, K, sa.group_all, False, sa.convs, sa.bns, neighbour_idx=nbr)
            tt = timed(fns, max(3, args.windows // 2), args.window / 3)
            levels[name] = {f"{k}_ms": round(v[0], 4) for k, v in tt.items()}
            levels[name].update({f"{k}_ms_spread": round(v[2] - v[1], 4) for k, v in tt.items()})
            levels[name]["rows"] = [B, 1 if sa.group_all else sa.npoint, xyz.shape[1] if sa.group_all else sa.nsample]
            xyz, pts = pred._fused(i, d, xyz, pts, centre, nbr)
            xyz, pts = xyz.clone(), pts.clone()
    res["levels"] = levels
    fps = sum(v.get("fps_ms", 0.0) for v in levels.values())
    res["fps_ms"], res["fps_share_of_predictor"] = round(fps, 4), round(fps / mp, 3)
    doc = json.dumps(res, indent=1)
    print(doc, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
