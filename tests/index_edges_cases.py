"""The entries of tests/golden/index_edges.npz (oracle/make_index_edges.py: inputs and the reference's own outputs) in the form the
CPU oracle test and the GPU kernel test both run: the same cases, the same expected arrays, bit for bit."""
import numpy as np
import torch

FIXTURE = "index_edges.npz"
RADII = (0.05, 0.1, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.8)   # the issue's list; the fixture's rb_radii is checked against it
OTHER_BALL = (("be_empty", 0.2), ("be_under", 0.25), ("be_full", 1.0))
FPS = ("fd", "fo", "f1")


def _t(a):
    return torch.from_numpy(np.asarray(a))


def boundary(g, r):
    """-> xyz (1,M,3), new_xyz (1,1,3), [(nsample, the reference's list int64 (1,1,nsample))]: nothing cut off, then cut short"""
    tag = f"rb_{r}"
    full, cut = g[f"{tag}_idx"].astype(np.int64), g[f"{tag}_idx_cut"].astype(np.int64)
    return _t(g[f"{tag}_xyz"]), _t(g[f"{tag}_new_xyz"]), [(full.shape[-1], full), (cut.shape[-1], cut)]


def other_ball(g, tag):
    idx = g[f"{tag}_idx"].astype(np.int64)
    return _t(g[f"{tag}_xyz"]), _t(g[f"{tag}_new_xyz"]), idx.shape[-1], idx


def fps(g, tag):
    idx = g[f"{tag}_idx"].astype(np.int64)
    return _t(g[f"{tag}_xyz"]), idx.shape[-1], _t(g[f"{tag}_start"]), idx


def nan_padded(xyz, extra=7):
    """the cloud with `extra` NaN rows after it and the lengths that exclude them: a NaN distance passes !(d > r2), so a row read
    beyond a cloud's length shows up in the list"""
    B, N, _ = xyz.shape
    return torch.cat([xyz, torch.full((B, extra, 3), float("nan"))], 1).contiguous(), [N] * B
