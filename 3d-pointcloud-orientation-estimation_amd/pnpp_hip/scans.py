"""Device-side preparation of raw scans: what turns 10^4 .. 10^5 points of uneven density, with stray returns, an arbitrary offset
and size, into the clean, centred, unit-size cloud every model here was trained on.

`ScanPrep` chains the three standard steps -- voxel-grid downsample (ops.voxel_downsample), statistical outlier removal
(ops.remove_outliers), unit frame (ops.normalize_clouds) -- in that order, each skipped when its argument is None, and with
`resample=num` ends in the uniform (B, num, 3) batch the models take.  Ragged in, ragged out, nothing read back.  Nothing is prepared
unless asked: the loaders take `prepare=None` by default."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops

# DeviceCloudBank's draws count up from 1, SingleView's are 2^62 | i and 2^62 | 2^61 | i, Augment's 2^63 | i: the resampling draw of call
# i here is 2^60 | i, which has bits 61..63 clear and bit 60 set -- it meets none of them (the bank would need 2^60 draws to get there)
STREAM_BASE = 1 << 60


class Frame(NamedTuple):
    """x_scan = x' * scale[b] + centre[b] maps a prepared cloud back; yaw is invariant under both."""
    centre: torch.Tensor   # (B, 3) float32
    scale: torch.Tensor    # (B,) float32


class ScanPrep:
    """prep(xyz, lengths=None) -> (xyz', lengths', Frame(centre, scale)).

    grid / cell: the voxel step (one of them, or neither to skip it); outlier_k / outlier_std: the outlier step (outlier_k=None skips
    it); centre / scale: the unit frame (both None skips it: the frame is then zeros and ones).  resample=num draws `num` rows per
    cloud from the survivors through ops.subsample_points -- xyz' is (B, num, 3), lengths' all num -- with stream id 2^60 | i for call
    i, so a run is a function of `seed` and `draws`.  `last_lengths` keeps the survivor counts of the latest call on the device."""

    def __init__(self, grid=None, cell=None, outlier_k=16, outlier_std: float = 2.0, centre="centroid", scale="sphere", resample=None,
                 seed: int = 0):
        self.grid, self.cell, self.outlier_k, self.outlier_std = grid, cell, outlier_k, outlier_std
        self.centre, self.scale, self.seed = centre, scale, int(seed)
        if resample is not None and int(resample) < 1:
            raise ValueError(f"ScanPrep: resample={resample} must be a positive row count")
        self.resample = None if resample is None else int(resample)
        self.voxel = grid is not None or cell is not None
        self.frame = centre is not None or scale is not None
        ops.scan_plan((1, 1 << 24, 3), **self._plan_kwargs())   # checked once, on the host
        self.draws = 0
        self.last_lengths = None

    def _plan_kwargs(self):
        kw = dict(cell=self.cell, grid=self.grid, k=self.outlier_k, std_ratio=self.outlier_std)
        if self.frame:
            kw.update(centre=self.centre, scale=self.scale)
        return kw

    def prep(self, xyz, lengths=None):
        if self.resample is not None and (xyz.dim() != 3 or xyz.shape[2] != 3):
            raise ValueError(f"ScanPrep: resample= draws xyz rows only, the batch is {tuple(xyz.shape)}; estimate normals afterwards")
        ops.scan_plan(xyz.shape, lengths=lengths, **self._plan_kwargs())   # refuse before a draw is counted
        B, N = xyz.shape[0], xyz.shape[1]
        if self.voxel:
            xyz, lengths = ops.voxel_downsample(xyz, cell=self.cell, grid=self.grid, lengths=lengths)
        if self.outlier_k is not None:
            xyz, lengths = ops.remove_outliers(xyz, self.outlier_k, self.outlier_std, lengths)
        if self.frame:
            xyz, c, r = ops.normalize_clouds(xyz, lengths, self.centre, self.scale)
        else:
            c, r = xyz.new_zeros(B, 3), xyz.new_ones(B)
        if lengths is None:
            lengths = torch.full((B,), N, device=xyz.device, dtype=torch.int32)
        lengths = lengths.to(torch.int32)
        self.last_lengths = lengths
        if self.resample is not None:
            self.draws += 1
            xyz = ops.subsample_points(self.seed, STREAM_BASE | self.draws, xyz, lengths, self.resample)
            lengths = torch.full((B,), self.resample, device=xyz.device, dtype=torch.int32)
        return xyz, lengths, Frame(c, r)

    __call__ = prep
