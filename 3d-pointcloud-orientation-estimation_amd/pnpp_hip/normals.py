"""Surface normals for xyz-only clouds, on the device.

Every cloud that reaches this library is xyz only (the PLY readers keep three columns, DeviceCloudBank is (n, Lmax, 3), a sensor
scan has no normals), while the PointNet++ classifier and the six-channel PointNet take a normal per point.  `estimate_normals`
closes that gap in one launch (ops.estimate_normals): the neighbour search of ops.knn with every point as a query, and in the same
kernel the float64 covariance of each neighbourhood, its smallest eigenvector and the surface variation.

The definition (include/pnpp_hip.h: pnpp_estimate_normals) for cloud b, point i, neighbourhood size k:
    neighbours   row i of ops.knn(xyz, xyz, k, lengths) -- the point itself included;
    covariance   float64, d_j = p_j - p_i, m = mean d_j, C = mean d_j d_j^T - m m^T, eigenvalues l0 <= l1 <= l2;
    normal       a unit eigenvector of l0; its largest-magnitude component positive (lowest index among equals), then oriented
                 against the cloud's reference point r: s = n . (p_i - r), "away" flips when s < 0, "toward" when s > 0;
    curvature    max(l0, 0) / (l0 + l1 + l2); all k neighbours coincident: normal (0, 0, 0), curvature 0.
Results are detached float32 tensors: normals are data, not a differentiable op.  With `lengths` None or a device tensor a call
reads nothing back from the device and can be captured in torch.cuda.graph."""
from __future__ import annotations

import torch

from . import _lib as L
from . import ops
from .lengths import ragged_lengths

__all__ = ["estimate_normals", "with_normals", "reference_points"]


def reference_points(xyz: torch.Tensor, lengths=None) -> torch.Tensor:
    """(B, 3) float32: the mean of each cloud's valid rows (float64 sum, rounded once).  Device ops only, no read-back; rows at or beyond
    lengths[b] may hold anything, NaN included."""
    ops._need_gpu(xyz, "xyz")
    x = xyz.detach()
    B, N = x.shape[0], x.shape[1]
    if lengths is None:
        return x.double().mean(dim=1).float()
    n = ragged_lengths(lengths, B, N, x.device).clamp(1, N)
    valid = torch.arange(N, device=x.device)[None, :] < n[:, None]
    total = torch.where(valid[:, :, None], x, x.new_zeros(())).double().sum(dim=1)
    return (total / n[:, None].double()).float()


def _orientation(xyz: torch.Tensor, orient, lengths):
    """orient -> (mode, ref): "centroid" = away from reference_points; a (3,) or (B, 3) tensor = toward that viewpoint; None = the
    canonical sign."""
    if orient is None:
        return L.NORMALS_NONE, None
    if isinstance(orient, str):
        if orient != "centroid":
            raise ValueError(f"orient must be 'centroid', a viewpoint tensor of shape (3,) or (B, 3), or None; got {orient!r}")
        return L.NORMALS_AWAY, reference_points(xyz, lengths)
    if not isinstance(orient, torch.Tensor):
        raise TypeError(f"orient must be 'centroid', a viewpoint tensor or None, got {type(orient).__name__}")
    B = xyz.shape[0]
    if tuple(orient.shape) not in ((3,), (B, 3)):
        raise ValueError(f"a viewpoint must have shape (3,) or ({B}, 3), got {tuple(orient.shape)}")
    view = orient.detach().to(device=xyz.device, dtype=torch.float32)
    return L.NORMALS_TOWARD, view.expand(B, 3).contiguous()


def _run(xyz, k, orient, lengths, stride, curvature, neighbours):
    ops._need_gpu(xyz, "xyz")
    xyz = xyz.detach()
    mode, ref = _orientation(xyz, orient, lengths)
    return ops.estimate_normals(xyz, int(k), mode, ref, lengths, stride, curvature, neighbours)


def estimate_normals(xyz: torch.Tensor, k: int = 16, orient="centroid", lengths=None, curvature: bool = False, neighbours: bool = False):
    """xyz (B, N, 3) float32 -> normals (B, N, 3); with curvature=True also the (B, N) surface variation, with neighbours=True also the
    (B, N, k) int32 neighbour lists the normals were computed from (those of ops.knn(xyz, xyz, k, lengths)), in this order.
    3 <= k <= 128, k <= N.  lengths (B,): a ragged batch -- row b is the call on xyz[b:b+1, :lengths[b]] alone, bit for bit, and the
    rows at or beyond lengths[b] are zeros in every output."""
    out, curv, idx = _run(xyz, k, orient, lengths, 3, curvature, neighbours)
    extra = tuple(t for t in (curv, idx) if t is not None)
    return (out, *extra) if extra else out


def with_normals(xyz: torch.Tensor, k: int = 16, orient="centroid", lengths=None) -> torch.Tensor:
    """xyz (B, N, 3) -> (B, N, 6): the points in columns 0-2 (bit for bit) and their normals in 3-5, written by the kernel itself --
    the rows Augment turns and, transposed, the input of PointNetPlusPlusCls and the six-channel PointNet."""
    return _run(xyz, k, orient, lengths, 6, False, False)[0]
