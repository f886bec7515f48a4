"""Device-side single-view scan simulation: what a sensor on one side of an object sees of it.

The reference trains on samplings that cover the whole surface (its ModelNet-style sets), and so do synthetic.py and DeviceCloudBank.
`SingleView` removes, per cloud and call, the points a viewer at infinity cannot see -- an orthographic depth buffer over the view plane
(ops.view_clouds, one launch, nothing read back) -- and returns a ragged batch, or with `resample=num` a uniform one drawn from the
survivors.  The cloud is not moved, so its orientation targets stay what they were; Augment, applied afterwards, turns both.  Nothing is
viewed unless asked: the loaders take `view=None` by default."""
from __future__ import annotations

import torch

from . import ops

STREAM_BASE = 1 << 62       # DeviceCloudBank draws count up from 1 and Augment's calls from 2^63: the three families never meet
RESAMPLE_BASE = STREAM_BASE | (1 << 61)   # the draw that follows call i of a resampling view


class SingleView:
    """view(xyz, lengths=None, view_dirs=None, index=False) -> (xyz', lengths'[, index]), or xyz' (B, resample, 3) alone with resample=.

    A run is a function of `seed` and `draws` (calls so far): call i uses stream id 2^62 | i.  elevation=(lo, hi) in radians is the
    range the viewing elevation is drawn from (the azimuth is uniform); resolution=None sizes the depth buffer at about one point per
    cell, min(128, ceil(sqrt(N))); a point covers the (2 splat + 1)^2 cells around its own and is visible within thickness x extent
    of the nearest depth there; drop thins the visible points by a per-cloud ratio uniform in [0, drop); a cloud left with fewer
    than min_keep points passes through whole (lengths.sa_minimum_length gives what a model's first level needs).  view_dirs (B,3)
    fixes the directions (towards the viewer), or (B,2) [azimuth, elevation].  `last_params` (B,8) = [v_x, v_y, v_z, azimuth,
    elevation, cell, kept, passed_through] of the latest call stays on the device."""

    def __init__(self, seed: int = 0, elevation=ops.VIEW_ELEVATION, resolution=None, splat: int = 1, thickness: float = 0.1,
                 drop: float = 0.0, min_keep: int = 1, resample=None):
        self.seed, self.elevation, self.resolution, self.splat = int(seed), tuple(elevation), resolution, splat
        self.thickness, self.drop, self.min_keep = thickness, drop, min_keep
        if resample is not None and int(resample) < 1:
            raise ValueError(f"SingleView: resample={resample} must be a positive row count")
        self.resample = None if resample is None else int(resample)
        ops.view_plan((1, max(int(min_keep), 1), 3), resolution, splat, thickness, elevation, drop, min_keep)   # checked once, on the host
        self.draws = 0
        self.last_params = None

    def _plan_kwargs(self):
        return dict(resolution=self.resolution, splat=self.splat, thickness=self.thickness, elevation=self.elevation, drop=self.drop,
                    min_keep=self.min_keep)

    def view(self, xyz, lengths=None, view_dirs=None, index: bool = False):
        dirs = view_dirs if view_dirs is not None and view_dirs.shape[-1] == 3 else None
        angles = view_dirs if view_dirs is not None and dirs is None else None
        if self.resample is not None and (xyz.dim() != 3 or xyz.shape[2] != 3):
            raise ValueError(f"SingleView: resample= draws xyz rows only, the batch is {tuple(xyz.shape)}; estimate normals after the view")
        if self.resample is not None and index:
            raise ValueError("SingleView: index= belongs to the ragged result; a resampled batch has no source rows to report")
        ops.view_plan(xyz.shape, lengths=lengths, view_dirs=dirs, angles=angles, **self._plan_kwargs())   # refuse before a draw is counted
        self.draws += 1
        res = ops.view_clouds(xyz, self.seed, STREAM_BASE | self.draws, lengths, view_dirs=dirs, angles=angles, index=index,
                              **self._plan_kwargs())
        self.last_params = res[2]
        if self.resample is not None:
            return ops.subsample_points(self.seed, RESAMPLE_BASE | self.draws, res[0], res[1], self.resample)
        return (res[0], res[1], res[3]) if index else (res[0], res[1])

    __call__ = view
