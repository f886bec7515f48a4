#!/usr/bin/env python
"""Writes tests/golden/mvm_decode.npz: seeded mixture parameters and the reference's own mvm_density_on_grid
(models/pointnet_pp_mvM.py of the reference checkout, loaded by path) evaluated on them in float64 on the CPU, at the grid sizes the
decode tests use.  Runs on a CPU box that has the reference:

    python tools/make_golden_decode.py /path/to/reference

kappa stays at or below 80: the reference's formula exp(kappa cos) / I0(kappa) is finite in float64 up to kappa ~ 700.
The fixture holds data only (inputs and recorded results)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMS = (9, 65, 360)


def load_ref(ref_root):
    sys.path.insert(0, os.path.abspath(ref_root))   # the module imports its siblings relatively: it is loaded as models.pointnet_pp_mvM
    try:
        m = importlib.import_module("models.pointnet_pp_mvM")
    finally:
        sys.path.pop(0)
    assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_root)), m.__file__
    return m


def inputs(B=4, K=4, seed=20240607):
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-np.pi, np.pi, (B, K))
    kappa = np.exp(rng.uniform(np.log(0.5), np.log(80.0), (B, K)))
    weight = rng.dirichlet(np.ones(K), B)
    mu[0], kappa[0] = [0.0, np.pi, 1.0, -2.0], [20.0, 20.0, 5.0, 1.0]   # a peak at 0 and one at pi: the wrap
    return mu.astype(np.float32), kappa.astype(np.float32), weight.astype(np.float32)


def main():
    ref = load_ref(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PNPP_REFERENCE", "../reference"))
    mu, kappa, weight = inputs()
    out = {"mu": mu, "kappa": kappa, "weight": weight, "nums": np.asarray(NUMS)}
    t = lambda a: torch.from_numpy(a).double()
    for num in NUMS:
        theta, p = ref.mvm_density_on_grid(t(mu), t(kappa), t(weight), num=num)
        assert p.dtype == torch.float64 and theta.shape == (num - 1,)
        out[f"theta_{num}"], out[f"density_{num}"] = theta.numpy(), p.numpy()
    path = os.path.join(ROOT, "tests", "golden", "mvm_decode.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
