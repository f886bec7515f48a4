#!/usr/bin/env python3
"""Writes tests/golden/pointnet_infer.npz: the reference's own vanilla PointNet (models/pointnet.py of the reference checkout, loaded
by path) run in float64 EVAL mode on seeded weights, randomised BatchNorm parameters / running statistics and seeded inputs, 8
clouds of 300 points (not a multiple of any tile).  Runs on a CPU box that has the reference:

    python tools/make_golden_pointnet_infer.py /path/to/reference

Cases: "ft" PointNet(feature_transform=True), "noft" PointNet(feature_transform=False) and "enc6" PointNetEncoder(global_feat=False,
feature_transform=True, channel=6).  The conv / linear weights are those of torch.manual_seed(SEED) followed by the constructor
(NSAMP sampled positions per weight are stored, "<case>.ws", so that a seeding drift is reported as such); every BatchNorm's weight,
bias, running_mean and running_var are randomised as tests/test_gpu_inference.py::_randomise does (running_var log-uniform in
[0.05, 2]), rounded to bfloat16-representable values so that two bytes each store them exactly, and stored in full as their bit
patterns: "<case>.bn" is the concatenation over the BatchNorm modules in named_modules() order of [weight, bias, running_mean,
running_var].  The encoder case draws from the same BN_SEED as "ft", whose first modules are the same, so it reads the head of
"ft.bn" and stores none of its own (4 clouds there; the file has a size limit).  Stored per case: x, out (the encoder's (B, 1088, N)
output at sampled positions), trans, trans_feat (float32 storage; the encoder's at sampled positions) and the (B, 1024) global
feature."""
import importlib.util
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pointnet_infer.npz")
B, N, NSAMP = 8, 300, 8
SEEDS = {"ft": 21, "noft": 22, "enc6": 23}
BN_SEED = 121


def load_ref(ref_root):
    spec = importlib.util.spec_from_file_location("ref_pointnet", os.path.join(ref_root, "models", "pointnet.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def randomise(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                n = m.num_features
                m.weight.copy_(0.5 + torch.rand(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(n, generator=g))
                m.running_var.copy_(torch.exp(math.log(0.05) + torch.rand(n, generator=g) * (math.log(2.0) - math.log(0.05))))
                for t in (m.weight, m.bias, m.running_mean, m.running_var):
                    t.copy_(t.bfloat16().float())
    return model


def bn_bits(model):
    parts = []
    for m in model.modules():
        if isinstance(m, nn.BatchNorm1d):
            parts += [t.detach().bfloat16().view(torch.int16) for t in (m.weight, m.bias, m.running_mean, m.running_var)]
    return torch.cat(parts).numpy().view(np.uint16)


def positions(p, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, p.numel(), (min(NSAMP, p.numel()),), generator=g).numpy()


def run_case(ref, tag, out):
    seed = SEEDS[tag]
    torch.manual_seed(seed)
    if tag == "enc6":
        model = ref.PointNetEncoder(global_feat=False, feature_transform=True, channel=6)
    else:
        model = ref.PointNet(feature_transform=tag == "ft")
    randomise(model, BN_SEED)
    out[f"{tag}.seed"] = np.array(seed)
    ws = []
    for i, (n, p) in enumerate(model.named_parameters()):
        if p.dim() > 1:   # conv / linear weights: sampled positions of the seeded initialisation (positions(p, index in named_parameters()))
            ws.append(p.detach().flatten()[positions(p, i)])
    out[f"{tag}.ws"] = torch.cat(ws).numpy()
    if tag != "enc6":
        out[f"{tag}.bn"] = bn_bits(model)
    else:
        assert np.array_equal(bn_bits(model), out["ft.bn"][:bn_bits(model).size])
    model = model.double().eval()
    g = torch.Generator().manual_seed(1000 + seed)
    caught = {}
    with torch.no_grad():
        if tag == "enc6":
            x = torch.randn(4, 6, N, generator=g).double()
            o, trans, tf = model(x)
            flat = o.flatten()
            pos = torch.randint(0, flat.numel(), (1024,), generator=torch.Generator().manual_seed(5)).numpy()
            out[f"{tag}.out_pos"], out[f"{tag}.out_s"] = pos.astype(np.int32), flat[pos].numpy()
            out[f"{tag}.out_absmax"] = np.array(float(flat.abs().max()))
            out[f"{tag}.global"] = o[:, :1024, 0].float().numpy()
            tpos = torch.randint(0, tf.numel(), (1024,), generator=torch.Generator().manual_seed(6)).numpy()
            out[f"{tag}.tf_pos"], out[f"{tag}.tf_s"] = tpos.astype(np.int32), tf.flatten()[tpos].numpy()
            out[f"{tag}.tf_absmax"] = np.array(float(tf.abs().max()))
            tf = None
        else:
            x = torch.randn(B, N, 3, generator=g).double()
            hook = model.encoder.register_forward_hook(lambda m, i, r: caught.update(r=r))
            o = model(x)
            hook.remove()
            gf, trans, tf = caught["r"]
            out[f"{tag}.out"] = o.numpy()
            out[f"{tag}.global"] = gf.float().numpy()
    out[f"{tag}.x"] = x.float().numpy()   # exactly representable: drawn in float32
    out[f"{tag}.trans"] = trans.numpy()
    if tf is not None:
        out[f"{tag}.trans_feat"] = tf.float().numpy()


def main():
    ref = load_ref(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PNPP_REFERENCE", "../reference"))
    torch.set_num_threads(8)
    out = {}
    for tag in SEEDS:
        run_case(ref, tag, out)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
