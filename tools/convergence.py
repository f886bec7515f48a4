#!/usr/bin/env python3
"""Does the path LEARN?  Trains the drop-in single-peak von-Mises model and the 8-direction model with the drop-in trainer (hipGraph
step, device-side centre sampling, FlatAdam) on generated clouds and records the loss curves and, on held-out clouds, the angular
error of the predicted orientation.

The bench's synthetic clouds (a box rotated about +Y) are symmetric under a half turn, so their yaw is observable only
modulo 180 degrees and no single-peak predictor can do better than chance on the sign.  The clouds here are the same recipe with
the box tapered towards its front (a wedge: 0.4 of the width at the front, full width at the back), which makes the yaw observable.

The multi-peak model has a mode of its own, --multi-peak: as the reference writes it (reproduced here), its mu head is
zero-initialised, which puts every component on the (c, s) = (1, 0) fallback whose gradient is zero, and match_loss normalises by
the weight of the first K components only, so the optimiser reaches loss 0 by moving the mixture weight to the unmatched components.
--multi-peak trains PointNetPPMvM twice from the same seed, that way (match_loss, mu_init="reference") and on the mixture KL of the
whole prediction (grid_kl, mu_init="spread"), on wedges (one valid heading) mixed with the same box without the taper (two:
front and back), and reports what Predictor.orientation + AngularErrors find on held-out clouds of each kind.

    python tools/convergence.py [--clouds 8192] [--epochs 40] > profiles/<round>_convergence.json
    python tools/convergence.py --augment > profiles/augment_convergence.json
    python tools/convergence.py --schedule > profiles/optim_convergence.json
    python tools/convergence.py --multi-peak > profiles/mvm_grid_kl_convergence.json

--schedule trains the single-peak model twice from the same initial state: as above, and with trainer.fit's optimiser options (linear
warm-up then cosine, decoupled weight decay on conv / linear weights only, averaged weights).  Both runs report the validation curve, its
swing over the last ten epochs, and the angular error on a third split (wedge_clouds(1024, N, 3)) that no checkpoint selection has seen.

--augment trains the single-peak model twice from the same initial state, on the same clouds: as above, and with the training loader
wrapped in trainer.AugmentedLoader (pnpp_hip.augment.Augment: a fresh yaw per cloud and draw, mu moved along); held-out clouds untouched.

    python tools/convergence.py --views > profiles/views_convergence.json
    python tools/convergence.py --scan-prep > profiles/scans_convergence.json

--views trains the single-peak model twice from the same initial state, on the same clouds: on the whole clouds, and with the training
loader wrapped in trainer.ViewLoader (pnpp_hip.views.SingleView: a fresh viewing direction per cloud and draw, the hidden side removed,
resampled to --points).  Both models are then asked for the orientation of the held-out clouds whole and as one viewer sees them (one
fixed view per held-out cloud, the same for both models).
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd"))

import torch  # noqa: E402


def wedge_clouds(B, N, seed, taper=True):
    """-> xyz (B,N,3), mu (B,), forward axis (B,3): tapered box, random yaw about +Y, canonical forward axis (0,0,-1).
    taper=False: the plain box, symmetric under a half turn."""
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand(B, N, 3, generator=g) * 2 - 1) * torch.tensor([0.6, 0.3, 1.0])
    if taper:
        p[:, :, 0] *= 0.4 + 0.6 * (p[:, :, 2] + 1.0) / 2.0      # narrow at z = -1 (the front), full width at the back
    th = torch.rand(B, generator=g) * (2 * math.pi)
    c, s = torch.cos(th), torch.sin(th)
    R = torch.zeros(B, 3, 3)
    R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = c, s, 1.0, -s, c
    xyz = torch.einsum("bnj,bij->bni", p, R).contiguous()
    f = torch.einsum("bij,j->bi", R, torch.tensor([0.0, 0.0, -1.0]))
    return xyz.float(), torch.atan2(f[:, 0], -f[:, 2]).float(), f.float()


def raw_scans(dense, seed):
    """Clean clouds (B,M,3) -> (xyz (B,Lmax,3) zero-padded, lengths (B,) int32) as a sensor might deliver them: 5 % of the rows
    replaced by uniform strays in twice the cloud's box, the low-x half thinned to half the sampling density of the other, then a
    scale in [0.5, 2] and an offset in [-5, 5]^3 per cloud."""
    g = torch.Generator().manual_seed(seed)
    B, M, _ = dense.shape
    lo, hi = dense.amin(1, keepdim=True), dense.amax(1, keepdim=True)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    stray = torch.rand(B, M, generator=g) < 0.05
    pts = torch.where(stray[..., None], mid + (torch.rand(B, M, 3, generator=g) * 2 - 1) * 2 * half, dense)
    keep = ~((dense[..., 0] < mid[..., 0]) & (torch.rand(B, M, generator=g) < 0.5) & ~stray)
    pts = pts * (0.5 + 1.5 * torch.rand(B, 1, 1, generator=g)) + (torch.rand(B, 1, 3, generator=g) * 2 - 1) * 5
    order = torch.sort((~keep).to(torch.uint8), dim=1, stable=True).indices
    lengths = keep.sum(1)
    out = torch.gather(pts, 1, order[..., None].expand(-1, -1, 3)) * (torch.arange(M)[None, :] < lengths[:, None])[..., None]
    return out[:, :int(lengths.max())].contiguous().float(), lengths.to(torch.int32)


def ang_err_deg(a, b):
    d = (a - b + math.pi) % (2 * math.pi) - math.pi
    return d.abs() * 180.0 / math.pi


def multi_peak_clouds(B, N, seed):
    """Half wedges (K_gt = 1: the heading), half plain boxes (K_gt = 2: front and back, weights 1/2), kappa 8, shuffled.
    -> xyz (B,N,3), vm_gt (B,4,3), K_gt (B,) int32, kind (B,) int32 (0 wedge, 1 box)"""
    half = B // 2
    xw, mw, _ = wedge_clouds(half, N, seed)
    xb, mb, _ = wedge_clouds(B - half, N, seed + 100, taper=False)
    vm = torch.zeros(B, 4, 3)
    vm[:half, 0] = torch.stack([mw, torch.full_like(mw, 8.0), torch.ones_like(mw)], 1)
    back = (mb + 2 * math.pi) % (2 * math.pi) - math.pi        # mb - pi wrapped into [-pi, pi)
    vm[half:, 0] = torch.stack([mb, torch.full_like(mb, 8.0), torch.full_like(mb, 0.5)], 1)
    vm[half:, 1] = torch.stack([back, torch.full_like(mb, 8.0), torch.full_like(mb, 0.5)], 1)
    K = torch.cat([torch.ones(half, dtype=torch.int32), torch.full((B - half,), 2, dtype=torch.int32)])
    kind = (K - 1).clone()
    order = torch.randperm(B, generator=torch.Generator().manual_seed(seed + 7))
    return torch.cat([xw, xb])[order].contiguous(), vm[order].contiguous(), K[order].contiguous(), kind[order].contiguous()


def derived_targets(data, dev, points):
    """The training table of a user who has one heading per cloud and no K: the clouds go into a DeviceCloudBank, bank.symmetry reads
    each cloud's yaw symmetry from its own geometry and symmetric_targets turns heading + order into (vm_gt, K_gt).
    -> (the data with the derived table, the share of clouds whose derived order equals the generator's K)"""
    from dataloader_common import DeviceCloudBank
    from pnpp_hip.symmetry import symmetric_targets
    xyz, vm, K, kind = data
    sym = DeviceCloudBank(list(xyz.numpy()), dev).symmetry(num_points=points)
    vm_d, K_d = symmetric_targets(vm[:, 0, 0].to(dev), sym)
    orders = sym.order.cpu()
    return (xyz, vm_d.cpu().contiguous(), K_d.cpu().contiguous(), kind), {
        "order_equals_generator": round(float((orders == K).float().mean()), 4),
        "order_histogram": {str(int(o)): int((orders == o).sum()) for o in orders.unique()},
        "wedge_order_1": round(float((orders[kind == 0] == 1).float().mean()), 4),
        "box_order_2": round(float((orders[kind == 1] == 2).float().mean()), 4)}


def multi_peak(args, dev):
    """match_loss + mu_init="reference" against grid_kl + mu_init="spread", same seed, same clouds.  --derived-gt: the training table
    comes from derived_targets; the held-out errors are still measured against the generator's own targets."""
    from models.pointnet_pp_mvM import PointNetPPMvM
    from pnpp_hip import ops, sampling, trainer
    from pnpp_hip.decode import AngularErrors
    from pnpp_hip.inference import Predictor
    train = multi_peak_clouds(args.clouds, args.points, 1)
    held = multi_peak_clouds(2048, args.points, 2)
    out = {"workload": f"PointNetPPMvM (max_K 4) on tapered boxes (K_gt 1) mixed half and half with plain boxes (K_gt 2: front and back, "
                       f"kappa 8, weights 1/2), N={args.points}, batch {args.batch}, {args.clouds} training / 2048 held-out clouds, "
                       f"{args.epochs} epochs, Adam lr 1e-3, clip 1.0, device-side centre sampling, hipGraph step; held-out errors by "
                       f"Predictor.orientation + AngularErrors (decode: num 360, rel_height 0.1), label 0 = wedge, 1 = box",
           "runs": {}}
    if args.derived_gt:
        train, out["derived_gt"] = derived_targets(train, dev, args.points)
        out["workload"] += "; TRAINING targets derived from the clouds (bank.symmetry, 72 angles, tol 1.3 -> symmetric_targets)"
    losses = {"match": lambda m, b: ops.match_loss(*m(b[0]), b[1], b[2]), "grid-kl": lambda m, b: m.grid_kl(b[0], b[1], b[2])}
    for loss_name, mu_init in (("match", "reference"), ("grid-kl", "spread")):
        torch.manual_seed(42)
        sampling.reset(0)
        model = PointNetPPMvM(sampler="device", mu_init=mu_init).to(dev)
        loaders = {"train": trainer.SyntheticLoader(list(train[:3]), args.batch, True, dev),
                   "val": trainer.SyntheticLoader(list(held[:3]), args.batch, False, dev)}
        hist, best, best_ep = trainer.fit(model, losses[loss_name], loaders, args.epochs, 1e-3, dev, clip_norm=1.0, label=loss_name,
                                          log=lambda *_: None)
        model.eval()
        pred, errs = Predictor(model), AngularErrors(n_labels=2)
        stats = {"mu": [], "kappa": [], "weight": []}
        with torch.no_grad():
            for i in range(0, 2048, args.batch):
                xyz, vm, K, kind = (t[i:i + args.batch].to(dev) for t in held)
                errs.update(pred.orientation(xyz), vm_gt=vm, K_gt=K, labels=kind)
                for name, t in zip(stats, pred(xyz)):
                    stats[name].append(t.cpu())
        mu, kappa, weight = (torch.cat(v) for v in stats.values())
        summary = errs.summary()

        def entry(e):
            r = lambda v: None if v is None else round(v, 3)
            return {"n": e["n"], "excluded": e["excluded"], "mode_count_rate": r(e["count_ok_rate"]),
                    "top1_deg": {k: r(v) for k, v in e["top1"].items()}, "cover_deg": {k: r(v) for k, v in e["cover"].items()}}

        out["runs"][f"{loss_name}+{mu_init}"] = {
            "train_loss": [round(v, 4) for v in hist["train"]], "val_loss": [round(v, 4) for v in hist["val"]], "best_val_epoch": best_ep,
            "steps": hist["steps"], "train_seconds_per_epoch": round(sum(hist["seconds"]["train"]) / args.epochs, 3),
            "held_out": {"wedge": entry(summary["labels"][0]), "box": entry(summary["labels"][1]), "overall": entry(summary["overall"])},
            "predicted_on_held_out": {"mu_abs_max": round(float(mu.abs().max()), 6), "mu_std_over_clouds": round(float(mu.std(0).mean()), 4),
                                      "mean_kappa_per_component": [round(float(v), 3) for v in kappa.mean(0)],
                                      "mean_weight_per_component": [round(float(v), 4) for v in weight.mean(0)]}}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=8192)
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16"], help="bf16: the opt-in bf16-operand MFMA mode")
    ap.add_argument("--augment", action="store_true", help="single-peak model only: without and with device-side yaw augmentation")
    ap.add_argument("--views", action="store_true", help="single-peak model only: trained on whole clouds and on single views of them")
    ap.add_argument("--scan-prep", action="store_true",
                    help="single-peak model only, trained as always: held-out clouds clean, as raw scans, and as raw scans through ScanPrep")
    ap.add_argument("--schedule", action="store_true",
                    help="single-peak model only: constant-rate Adam, then warm-up + cosine, decoupled weight decay and averaged weights")
    ap.add_argument("--multi-peak", action="store_true",
                    help="the multi-peak model only: match_loss + reference initialisation against grid_kl + spread initialisation")
    ap.add_argument("--derived-gt", action="store_true",
                    help="with --multi-peak: K and the peak set of the training clouds come from DeviceCloudBank.symmetry, not the generator")
    args = ap.parse_args()
    if args.multi_peak:
        from pnpp_hip import ops
        ops.set_matmul_precision(args.precision)
        return multi_peak(args, torch.device("cuda", 0))
    from models.pointnet_pp_8dir import DIRS_8, PointNetPP8Dir
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    from pnpp_hip import ops, sampling, trainer
    import synthetic
    dev = torch.device("cuda", 0)
    ops.set_matmul_precision(args.precision)
    xyz_tr, mu_tr, f_tr = wedge_clouds(args.clouds, args.points, 1)
    xyz_va, mu_va, f_va = wedge_clouds(1024, args.points, 2)
    out = {"workload": f"tapered-box clouds, N={args.points}, batch {args.batch}, {args.clouds} training / 1024 held-out clouds, "
                       f"{args.epochs} epochs, Adam lr 1e-3, device-side centre sampling, hipGraph step, matmul precision {args.precision}",
           "runs": {}}

    def single_peak(augment, fit_kw=None, unseen=None, views=False, viewed=None, scans=None):
        """train_single_peak_vonMises_KL.py's loss; augment: the training loader's batches in a fresh pose every draw; fit_kw: the
        optimiser options of trainer.fit; unseen: (xyz, mu) of a split no checkpoint selection has looked at; views: the training
        loader's clouds as one viewer sees them, a fresh direction every draw; viewed: the held-out clouds seen from one side; scans:
        {name: (xyz, mu)} further held-out sets of 1,024 clouds, each read by the last epoch's model and the best checkpoint"""
        torch.manual_seed(42)
        sampling.reset(0)
        model = PointNetPPVonMises(sampler="device").to(dev)
        kap = torch.full_like(mu_tr, 8.0)
        loaders = {"train": trainer.SyntheticLoader([xyz_tr, torch.stack([mu_tr, kap], 1)], args.batch, True, dev),
                   "val": trainer.SyntheticLoader([xyz_va, torch.stack([mu_va, torch.full_like(mu_va, 8.0)], 1)], args.batch, False, dev)}
        if augment:
            from pnpp_hip.augment import Augment
            loaders["train"] = trainer.AugmentedLoader(loaders["train"], Augment(seed=42), ("vm",))
        if views:
            from pnpp_hip.views import SingleView
            loaders["train"] = trainer.ViewLoader(loaders["train"], SingleView(seed=42, resample=args.points))
        loss = lambda m, b: ops.vm_head_kl_loss(m.features(b[0]), b[1][:, 0].contiguous(), b[1][:, 1].contiguous(), reduction="none")
        hist, best, best_ep = trainer.fit(model, loss, loaders, args.epochs, 1e-3, dev, label="von Mises KL", log=lambda *_: None,
                                          **(fit_kw or {}))
        model.eval()

        def held_out(xyz=xyz_va, mu_true=mu_va):
            errs, kaps = [], []
            with torch.no_grad():
                for i in range(0, 1024, args.batch):
                    mu, kappa = model(xyz[i:i + args.batch].to(dev))
                    errs.append(ang_err_deg(mu.cpu(), mu_true[i:i + args.batch]))
                    kaps.append(kappa.cpu())
            return torch.cat(errs), torch.cat(kaps)

        def summary(e):
            return {"mean": round(float(e.mean()), 2), "median": round(float(e.median()), 2),
                    "p90": round(float(e.kthvalue(int(0.9 * len(e))).values), 2)}

        e, k = held_out()                 # the LAST epoch's model (its validation KL swings from epoch to epoch at this learning rate)
        eu = held_out(*unseen)[0] if unseen is not None else None
        ev = held_out(viewed, mu_va)[0] if viewed is not None else None
        es = {name: summary(held_out(x, m)[0]) for name, (x, m) in (scans or {}).items()}
        model.load_state_dict(best)       # the checkpoint of the best validation epoch (trainer.fit keeps a copy)
        eb, kb = held_out()
        extra = {}
        if scans:
            extra = {"scan_angular_error_deg": {name: {"last_epoch": es[name], "best_checkpoint": summary(held_out(x, m)[0])}
                                                for name, (x, m) in scans.items()}}
        if viewed is not None:            # the same held-out clouds, one side of each
            extra = {"held_out_viewed_angular_error_deg": {"last_epoch": summary(ev), "best_checkpoint": summary(held_out(viewed, mu_va)[0])}}
        if unseen is not None:            # a third split: neither trained on nor used to pick the checkpoint
            last10 = hist["val"][-10:]
            extra = {"lr": hist["lr"], "averaged_weights": hist["ema"], "val_kl_swing_last_10_epochs": round(max(last10) - min(last10), 4),
                     "unseen_split_angular_error_deg": {"last_epoch": summary(eu), "best_checkpoint": summary(held_out(*unseen)[0])}}
        return {
            **extra,
            "train_kl": [round(v, 4) for v in hist["train"]], "val_kl": [round(v, 4) for v in hist["val"]], "best_val_epoch": best_ep,
            "steps": hist["steps"], "train_seconds_per_epoch": round(sum(hist["seconds"]["train"]) / args.epochs, 3),
            "held_out_angular_error_deg": {"mean": round(float(e.mean()), 2), "median": round(float(e.median()), 2),
                                           "p90": round(float(e.kthvalue(int(0.9 * len(e))).values), 2)},
            "held_out_mean_kappa": round(float(k.mean()), 2),
            "best_checkpoint": {"held_out_angular_error_deg": {"mean": round(float(eb.mean()), 2), "median": round(float(eb.median()), 2),
                                                               "p90": round(float(eb.kthvalue(int(0.9 * len(eb))).values), 2)},
                                "held_out_mean_kappa": round(float(kb.mean()), 2)}}

    if args.schedule:
        from pnpp_hip import optim
        unseen = wedge_clouds(1024, args.points, 3)[:2]
        out["workload"] += "; second run: AdamW weight decay 1e-2 on conv / linear weights, 5 % linear warm-up then cosine to 0.01 x, " \
                           "averaged weights (decay 0.999) for validation and the checkpoint; angular error also on a third, unseen split"
        out["runs"]["single_peak_vonMises_KL"] = single_peak(False, None, unseen)
        steps = args.epochs * ((args.clouds + args.batch - 1) // args.batch)
        kw = dict(weight_decay=1e-2, schedule=optim.Schedule.cosine(warmup=steps // 20, start_factor=0.1, min_factor=0.01), ema_decay=0.999)
        out["runs"]["single_peak_vonMises_KL_scheduled"] = single_peak(False, kw, unseen)
        print(json.dumps(out))
        return
    if args.scan_prep:
        from pnpp_hip.scans import ScanPrep
        dense, mu_s, _ = wedge_clouds(1024, 4 * args.points, 4)
        raw, raw_len = raw_scans(dense, 5)
        rd, ld = raw.to(dev), raw_len.to(dev)
        prep = ScanPrep(grid=32, outlier_k=8, outlier_std=1.0, resample=args.points, seed=7)
        first = ScanPrep(grid=32, outlier_k=8, outlier_std=1.0, centre=None, scale=None)   # "twice": a ragged cleaning pass in front
        again = ScanPrep(grid=32, outlier_k=8, outlier_std=1.0, resample=args.points, seed=7)
        prepared, survivors, twice = [], [], []
        for i in range(0, 1024, 128):
            chunk, lens = rd[i:i + 128].contiguous(), ld[i:i + 128].contiguous()
            prepared.append(prep(chunk, lens)[0].cpu())
            survivors.append(prep.last_lengths.cpu())
            twice.append(again(*first(chunk, lens)[:2])[0].cpu())
        clean = dense[:, :args.points].contiguous()
        sets = {"clean": (clean, mu_s),
                "clean_unit_frame": (ops.normalize_clouds(clean.to(dev))[0].cpu(), mu_s),   # what the frame alone costs this model
                "raw": (ops.subsample_points(7, 1, rd, ld, args.points).cpu(), mu_s),   # the same scans, resampled and nothing else
                "prepared": (torch.cat(prepared), mu_s),
                "prepared_twice": (torch.cat(twice), mu_s)}
        out["median_point_norm"] = {k: round(float(v[0].norm(dim=2).median()), 3) for k, v in sets.items()}
        out["workload"] += (f"; 1,024 further held-out clouds of {4 * args.points} points read three ways: clean ({args.points} of their rows), as "
                            f"raw scans (5 % uniform strays in twice the box, the low-x half at half density, scale 0.5..2, offset up to 5; "
                            f"{float(raw_len.float().mean()):.0f} rows on average) resampled to {args.points}, and the raw scans through "
                            f"ScanPrep(grid=32, outlier_k=8, outlier_std=1.0, resample={args.points}), which keeps "
                            f"{float(torch.cat(survivors).float().mean()):.0f} rows on average before resampling; also the clean clouds through "
                            f"normalize_clouds alone (clean_unit_frame) and the raw scans through a ragged pass of the same voxel and outlier steps "
                            f"in front of that ScanPrep (prepared_twice).  Not measured: real scans, "
                            f"and clouds above 2^17 points")
        out["runs"]["single_peak_vonMises_KL"] = single_peak(False, scans=sets)
        print(json.dumps(out))
        return
    if args.views:
        from pnpp_hip.views import SingleView
        held = SingleView(seed=7, resample=args.points)
        viewed = held(xyz_va.to(dev)).cpu()
        kept = held.last_params[:, 6].cpu()
        out["workload"] += (f"; second run: every training batch through SingleView(resample={args.points}) (defaults: elevation -30..60 degrees, "
                            f"resolution {ops.view_resolution(args.points)}, splat 1, thickness 0.1); held-out clouds whole and as one fixed view each, "
                            f"which keeps {float(kept.mean()) / args.points:.3f} of a cloud's points on average before resampling")
        out["runs"]["single_peak_vonMises_KL"] = single_peak(False, viewed=viewed)
        out["runs"]["single_peak_vonMises_KL_views"] = single_peak(False, views=True, viewed=viewed)
        print(json.dumps(out))
        return
    out["runs"]["single_peak_vonMises_KL"] = single_peak(False)
    if args.augment:
        out["runs"]["single_peak_vonMises_KL_augmented"] = single_peak(True)
        print(json.dumps(out))
        return

    # --- 8-direction soft-label cross entropy (train_8dir_KL.py's loss) ---
    torch.manual_seed(42)
    sampling.reset(0)
    model8 = PointNetPP8Dir(sampler="device").to(dev)
    p_tr, p_va = synthetic.dir8_soft_labels(f_tr, DIRS_8), synthetic.dir8_soft_labels(f_va, DIRS_8)
    loaders = {"train": trainer.SyntheticLoader([xyz_tr, p_tr], args.batch, True, dev),
               "val": trainer.SyntheticLoader([xyz_va, p_va], args.batch, False, dev)}
    loss8 = lambda m, b: ops.soft_ce(m(b[0]), b[1])
    hist8, state8, best8 = trainer.fit(model8, loss8, loaders, args.epochs, 1e-3, dev, label="8-dir soft CE", log=lambda *_: None)
    model8.eval()

    def top1():
        hit = 0
        with torch.no_grad():
            for i in range(0, 1024, args.batch):
                logits = model8(xyz_va[i:i + args.batch].to(dev)).cpu()
                hit += int((logits.argmax(1) == p_va[i:i + args.batch].argmax(1)).sum())
        return hit

    hit = top1()
    model8.load_state_dict(state8)
    hit_best = top1()
    ent = float(-(p_va * torch.log(p_va.clamp_min(1e-12))).sum(1).mean())     # the soft labels' own entropy: the loss floor
    out["runs"]["8dir_soft_CE"] = {"train_ce": [round(v, 4) for v in hist8["train"]], "val_ce": [round(v, 4) for v in hist8["val"]],
                                   "best_val_epoch": best8, "label_entropy_floor": round(ent, 4),
                                   "held_out_top1_direction_accuracy": round(hit / 1024, 4),
                                   "best_checkpoint": {"held_out_top1_direction_accuracy": round(hit_best / 1024, 4)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
