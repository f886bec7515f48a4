#!/usr/bin/env python3
"""Writes tests/golden/pointnet.npz: the reference's own vanilla PointNet (models/pointnet.py of the reference checkout, loaded by
path) run in float64 on seeded weights and inputs, 16 clouds of 256 points.  Runs on a CPU box that has the reference:

    python tools/make_golden_pointnet.py /path/to/reference

Cases: PointNet(feature_transform=True), PointNet(feature_transform=False) -- loss mse_rows(out, t).mean() + 0.001 x
feature_transform_reguliarzer(trans_feat) with an explicit dropout keep-mask -- and PointNetEncoder(global_feat=False,
feature_transform=True, channel=6) with loss sum(out * up).  Recorded per case: outputs (the encoder's as samples + norm), trans,
trans_feat, loss, per-parameter sampled gradients and norms, the seeded initial weights as samples, the running statistics after
the step and the eval-mode outputs after it.  Each case's model seed is the first from its list whose float64 run keeps every ReLU
input of the 16-row head / T-Net tail layers at least MARGIN away from 0, so that a float32 evaluation takes the same decisions."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pointnet.npz")
B, N, P_DROP, MARGIN, NSAMP = 16, 256, 0.4, 3e-5, 8


def load_ref(ref_root):
    spec = importlib.util.spec_from_file_location("ref_pointnet", os.path.join(ref_root, "models", "pointnet.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _Mask(nn.Module):
    def __init__(self, mask, p):
        super().__init__()
        self.mask, self.scale = mask, 1.0 / (1.0 - p)

    def forward(self, x):   # nn.Dropout's contract: the identity in eval mode
        return x * self.mask.to(x) * self.scale if self.training else x


def reg(t):
    k = t.shape[1]
    return (torch.bmm(t, t.transpose(1, 2)) - torch.eye(k, dtype=t.dtype)).flatten(1).norm(dim=1).mean()


def positions(p, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, p.numel(), (min(NSAMP, p.numel()),), generator=g).numpy()


def run_case(ref, tag, seed, out):
    """-> min |ReLU input| over the rows-of-16 layers of this case's float64 run."""
    torch.manual_seed(seed)
    if tag.startswith("enc6"):
        model = ref.PointNetEncoder(global_feat=False, feature_transform=True, channel=6)
    else:
        model = ref.PointNet(feature_transform=tag == "ft")
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    model = model.double().train()
    g = torch.Generator().manual_seed(1000 + seed)
    margin = [float("inf")]
    relu0 = F.relu

    def relu(x, inplace=False):
        if x.dim() == 2:
            margin[0] = min(margin[0], float(x.detach().abs().min()))
        return relu0(x, inplace=inplace)

    F.relu = relu
    try:
        if tag.startswith("enc6"):
            x = torch.randn(B, 6, N, generator=g, dtype=torch.float64)
            up = torch.randn(B, 1088, N, generator=g, dtype=torch.float64)
            o, trans, tf = model(x)
            loss = (o * up).sum()
        else:
            x = torch.randn(B, N, 3, generator=g, dtype=torch.float64)
            t = torch.randn(B, 3, generator=g, dtype=torch.float64)
            mask = (torch.rand(B, 256, generator=g) < 1.0 - P_DROP).to(torch.float64)
            model.dropout = _Mask(mask, P_DROP)
            caught = {}
            hook = model.encoder.register_forward_hook(lambda m, i, r: caught.update(r=r))
            o = model(x)
            hook.remove()
            _, trans, tf = caught["r"]
            loss = ((o - t) ** 2).mean(1).mean()
            if tf is not None:
                loss = loss + 0.001 * reg(tf)
            out[f"{tag}.t"], out[f"{tag}.mask"] = t.float().numpy(), mask.to(torch.uint8).numpy()
        loss.backward()
    finally:
        F.relu = relu0
    out[f"{tag}.seed"] = np.array(seed)
    out[f"{tag}.x"] = x.float().numpy()
    if tag.startswith("enc6"):
        flat = o.detach().flatten()
        pos = torch.randint(0, flat.numel(), (512,), generator=torch.Generator().manual_seed(5)).numpy()
        out[f"{tag}.out_pos"], out[f"{tag}.out_s"], out[f"{tag}.out_n"] = pos, flat[pos].numpy(), np.array(float(flat.norm()))
    else:
        out[f"{tag}.out"] = o.detach().numpy()
    out[f"{tag}.trans"] = trans.detach().numpy()
    if tf is not None:
        out[f"{tag}.trans_feat"] = tf.detach().float().numpy()   # float32 storage: the file stays small
    out[f"{tag}.loss"] = np.array(float(loss.detach()))
    for i, (n, p) in enumerate(model.named_parameters()):
        pos = positions(p, i)
        out[f"{tag}.gp.{n}"] = pos
        out[f"{tag}.gs.{n}"] = p.grad.detach().flatten()[pos].numpy()
        out[f"{tag}.gn.{n}"] = np.array(float(p.grad.detach().norm()))
        out[f"{tag}.init.{n}"] = init[n].flatten()[pos].numpy()
    for k, v in model.state_dict().items():
        if "running" in k:
            out[f"{tag}.after.{k}"] = v.float().numpy()
    model.eval()
    with torch.no_grad():
        ev = model(x)
        if tag.startswith("enc6"):
            ev = ev[0].flatten()
            out[f"{tag}.eval_s"] = ev[out[f"{tag}.out_pos"]].numpy()
        else:
            out[f"{tag}.eval_out"] = ev.numpy()
    return margin[0]


def main():
    ref = load_ref(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PNPP_REFERENCE", "../reference"))
    torch.set_num_threads(8)
    out = {}
    for tag in ("ft", "noft", "enc6"):
        for seed in range(100, 160):
            case = {}
            m = run_case(ref, tag, seed, case)
            print(f"{tag} seed {seed}: min |ReLU input| of the 16-row layers {m:.2e}")
            if m >= MARGIN:
                out.update(case)
                break
        else:
            raise SystemExit(f"{tag}: no seed with a ReLU margin of {MARGIN}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
