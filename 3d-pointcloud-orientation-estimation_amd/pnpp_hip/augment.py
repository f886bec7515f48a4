"""Device-side training augmentation: a fresh yaw about +Y per cloud and draw, with the orientation targets moved along.

The reference rotates its training sets offline (data_process/rotate_without_normals.py and the three GT writers), so a model
sees the same poses every epoch.  `Augment` turns every batch it is called on -- a DeviceCloudBank draw, a SyntheticLoader
batch, a ragged padded() batch -- in one launch (ops.augment_clouds): yaw by theta about +Y moves a forward axis f to R f, hence
mu = atan2(f_x, -f_z) to mu - theta (wrapped into (-pi, pi]); every peak of the multi-peak table shifts alike; 8-direction soft
labels are recomputed from the rotated axis.  Nothing is augmented unless asked: the loaders take `augment=None` by default."""
from __future__ import annotations

import torch

from . import ops

STREAM_BASE = 1 << 63   # DeviceCloudBank draws count up from 1: the two families of Philox counters never meet


class Augment:
    """augment(xyz, *targets, kinds=..., counts=None, lengths=None) -> (xyz', *targets').

    A run is a function of `seed` and `draws` (calls so far): call i uses stream id 2^63 | i.  scale=(lo, hi) and
    jitter=(sigma, clip) are off unless given.  kinds[i] names what targets[i] is -- "angle", "vm", "axis", "dir8" or "keep"
    (labels, kappa: passed through); `last_params` (B,4) = [cos, sin, scale, theta] of the latest call stays on the device."""

    def __init__(self, seed: int = 0, yaw: bool = True, scale=None, jitter=None):
        self.seed, self.yaw, self.scale, self.jitter = int(seed), bool(yaw), scale, jitter
        ops.augment_plan((1, 1, 3), (), (), None, scale, jitter)      # the ranges, checked once and on the host
        self.draws = 0
        self.last_params = None
        self._dirs8 = {}

    def _dirs(self, device):
        d = self._dirs8.get(device)
        if d is None:
            from models.pointnet_pp_8dir import DIRS_8
            d = self._dirs8[device] = DIRS_8.to(device=device, dtype=torch.float32).contiguous()
        return d

    def __call__(self, xyz, *targets, kinds, counts=None, lengths=None):
        ops.augment_plan(xyz.shape, targets, kinds, counts, self.scale, self.jitter)   # refuse before a draw is counted
        dirs8 = self._dirs(xyz.device) if "dir8" in kinds else None
        self.draws += 1
        out, outs, self.last_params = ops.augment_clouds(xyz, self.seed, STREAM_BASE | self.draws, targets, kinds, counts, lengths,
                                                         self.yaw, self.scale, self.jitter, dirs8)
        return (out, *outs)
