"""Yaw symmetry of a cloud from its own geometry, on the device.

A bank of posed xyz clouds has one heading per cloud and nothing that says which other headings are equally right; the multi-peak
targets (ops.mvm_grid_kl, match_loss) need exactly that.  The evidence is the cloud itself: under which rotations about +Y does it
map onto itself?  `yaw_profile` measures it -- the one-sided Chamfer distance between the cloud and its own turned copy at G angles,
B * G * N^2 exact float32 distances in one launch -- `yaw_symmetry` decides from it, and `symmetric_targets` turns a heading and a
decision into the (vm_gt, K_gt) table the losses and Augment take.

The definition (include/pnpp_hip.h: pnpp_yaw_profile, pnpp_yaw_symmetry; restated in tests/symmetry_ref.py) for cloud b:
    centre, rotate   q_i = (p_i.x - c.x, p_i.y, p_i.z - c.z);  x' = cs x + sn z, z' = cs z - sn x  (Augment's order), float32, unfused;
    profile          D[g] = mean_i min_j |rot_g(q_i) - q_j|^2 (exact_dist.h's direct form, lowest j among equals, float64 mean);
    floor            nu = the same at the identity with j != i: the mean squared distance to the nearest other point;
    symmetric        S[g] = D[g] + D[(G - g) % G] (the mirror index is the other direction), score[g] = S[g] / (2 nu);
    decision         bound = (2 nu) tol; order 0 (continuous) if S[g] <= bound for all g >= 1; else the largest m of `orders` dividing G
                     with S[k G / m] <= bound for k = 1..m-1; else 1.
Results are detached tensors.  With `lengths` None or a device tensor and the grid table warm (one earlier call with the same `num`
on the device) nothing is read back or uploaded, and a call can be captured in torch.cuda.graph."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .normals import reference_points

__all__ = ["yaw_profile", "yaw_symmetry", "symmetric_targets", "grid_table", "YawProfile", "YawSymmetry"]


class YawProfile(NamedTuple):
    distance: torch.Tensor                 # (B, G) D[b, g]
    floor: torch.Tensor                    # (B,)   nu[b]
    table: torch.Tensor                    # (G, 2) the (cos, sin) rows the kernel used
    nearest_dist: Optional[torch.Tensor]   # (B, G, N) float32, with nearest=True
    nearest_idx: Optional[torch.Tensor]    # (B, G, N) int32


class YawSymmetry(NamedTuple):
    order: torch.Tensor     # (B,) int32: 0 continuous, 1 none, m an m-fold symmetry
    count: torch.Tensor     # (B,) int32: the number of angles that follow
    angles: torch.Tensor    # (B, max(orders)) float32: 2 pi k / order for k < order, zeros beyond
    score: torch.Tensor     # (B, G) S / (2 nu)
    profile: YawProfile


_tables = {}


def grid_table(num: int, device) -> torch.Tensor:
    """(num, 2) float32 rows (cos, sin)(2 pi g / num): evaluated in float64 on the host and rounded once, the multiples of a quarter turn
    exactly (+-1, 0) and (0, +-1).  Cached per (num, device): the first call uploads, so make it before a graph capture."""
    if int(num) < 1:
        raise ValueError(f"num={num}: the grid needs at least one angle")
    device = torch.device(device)
    key = (int(num), str(device))
    t = _tables.get(key)
    if t is None:
        G = int(num)
        a = 2.0 * np.pi * np.arange(G, dtype=np.float64) / G
        tab = np.stack([np.cos(a), np.sin(a)], 1)
        for g in range(G):
            if (4 * g) % G == 0:   # a multiple of a quarter turn
                tab[g] = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[4 * g // G]
        t = torch.from_numpy(tab.astype(np.float32)).to(device)
        _tables[key] = t
    return t


def _centres(xyz, centre, lengths):
    B = xyz.shape[0]
    if isinstance(centre, str):
        if centre == "centroid":
            return reference_points(xyz, lengths)
        if centre == "origin":
            return xyz.new_zeros(B, 3)
        raise ValueError(f"centre must be 'centroid', 'origin' or a (B, 3) tensor, got {centre!r}")
    if not isinstance(centre, torch.Tensor):
        raise TypeError(f"centre must be 'centroid', 'origin' or a tensor, got {type(centre).__name__}")
    if tuple(centre.shape) != (B, 3):
        raise ValueError(f"a centre tensor must have shape ({B}, 3), got {tuple(centre.shape)}")
    return centre.detach().to(device=xyz.device, dtype=torch.float32).contiguous()


def _prepare(xyz, num, angles, centre, lengths):
    ops._need_gpu(xyz, "xyz")
    xyz = xyz.detach()
    if angles is None:
        table = grid_table(num, xyz.device)
    else:
        ops._need_gpu(angles, "angles")
        a = angles.detach().reshape(-1).to(torch.float32)
        table = torch.stack([torch.cos(a), torch.sin(a)], 1).contiguous()
    return xyz, table, _centres(xyz, centre, lengths)


def yaw_profile(xyz: torch.Tensor, num: int = 72, angles=None, centre="centroid", lengths=None, nearest: bool = False) -> YawProfile:
    """xyz (B, N, 3) float32 -> YawProfile at the uniform grid of `num` angles, or at `angles` (a device tensor of radians, any length;
    its table is cos / sin in float32 on the device, nothing snapped).  centre: "centroid" (the float64 mean of the valid rows, rounded
    to float32), "origin" or a (B, 3) tensor; only x and z are used.  nearest=True also returns every query's nearest candidate and its
    squared distance per angle.  lengths (B,): a ragged batch -- row b is the call on xyz[b:b+1, :lengths[b]] alone, bit for bit."""
    xyz, table, c = _prepare(xyz, num, angles, centre, lengths)
    r = ops.yaw_profile(xyz, c, table, lengths, nearest)
    return YawProfile(r["distance"], r["floor"], table, r["nearest_dist"], r["nearest_idx"])


def yaw_symmetry(xyz: torch.Tensor, num: int = 72, tol: float = 1.3, orders=(2, 3, 4, 6, 8), centre="centroid",
                 lengths=None) -> YawSymmetry:
    """xyz (B, N, 3) float32 -> YawSymmetry on the uniform grid of `num` angles.  tol: a rotation is a symmetry when the symmetric Chamfer
    distance stays within tol times twice the floor (1.3 sits between the 1.09 true symmetries reach at N = 1024 and the 1.64 of the
    nearest false one).  orders: the candidate orders; those that do not divide `num` cannot be tested on this grid and are left out."""
    orders = tuple(int(m) for m in orders)
    if any(m < 2 for m in orders):
        raise ValueError(f"orders={orders}: a candidate order is at least 2")
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"tol={tol} must be a finite, non-negative number")
    xyz, table, c = _prepare(xyz, num, None, centre, lengths)
    G = table.shape[0]
    r = ops.yaw_profile(xyz, c, table, lengths, decide=(tol, [m for m in orders if G % m == 0], max(orders, default=1)))
    profile = YawProfile(r["distance"], r["floor"], table, None, None)
    return YawSymmetry(r["order"], r["count"], r["angles"], r["score"], profile)


def symmetric_targets(mu: torch.Tensor, sym, kappa: float = 8.0, max_K: int = 4):
    """A heading per cloud and its symmetry -> (vm_gt (B, max_K, 3) rows [mu, kappa, weight], K_gt (B,) int32): the table ops.mvm_grid_kl
    and match_loss take and Augment turns.  sym: a YawSymmetry or its (B,) order tensor.  Peak k of an order-m cloud is mu - 2 pi k / m
    wrapped into (-pi, pi] as Augment wraps (float64, one conditional + 2 pi), weight 1 / m; order 1 is one peak.  A continuous cloud
    (order 0) or an order above max_K gives the reference's K = 0 row: one peak at mu with kappa = 0.  Torch ops only, on mu's device."""
    order = (sym.order if isinstance(sym, YawSymmetry) else sym).to(device=mu.device, dtype=torch.int64)
    if mu.dim() != 1 or order.shape != mu.shape:
        raise ValueError(f"mu (B,) and the orders (B,) must agree, got {tuple(mu.shape)} and {tuple(order.shape)}")
    peaked = (order >= 1) & (order <= max_K)
    K = torch.where(peaked, order, torch.ones_like(order))
    k = torch.arange(max_K, device=mu.device)
    v = mu.double()[:, None] - (2.0 * math.pi) * k.double()[None, :] / K.double()[:, None]
    v = torch.where(v <= -math.pi, v + 2.0 * math.pi, v)
    real = k[None, :] < K[:, None]
    zero = mu.new_zeros(())
    kap = torch.where(peaked, mu.new_full((), float(kappa)), zero)
    vm = torch.stack([torch.where(real, v.to(mu.dtype), zero), torch.where(real, kap[:, None], zero),
                      torch.where(real, (1.0 / K.double()).to(mu.dtype)[:, None], zero)], -1)
    return vm, K.to(torch.int32)
