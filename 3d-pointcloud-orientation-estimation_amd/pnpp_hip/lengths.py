"""Per-cloud lengths of a ragged batch: a padded (B, n_pts, ...) tensor plus `lengths` (B,), cloud b holding its first lengths[b] rows.
Shared by the point transformer (pnpp_hip.transformer), the set-abstraction models (pnpp_hip.ops, models.pointnet_pp_*) and the
vanilla PointNet (models.pointnet), whose kernels work on the PACKED valid rows and read the lengths' prefix sum (packed_lengths)."""
from typing import NamedTuple, Optional

import torch


def check_lengths(lengths, B: int, n_pts: int, minimum: int = 1) -> torch.Tensor:
    """Host-side validation of a ragged batch's per-cloud lengths, given as a list (or anything torch.as_tensor takes) or a CPU
    tensor: integer dtype, shape (B,), minimum <= lengths[b] <= n_pts (minimum: what the consumer's first level needs, see
    sa_minimum_length; at least 1).  -> the values as a CPU int32 tensor.  A violation raises ValueError naming the offending cloud.
    Runs without a GPU."""
    t = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths)
    if t.is_cuda:
        raise ValueError("check_lengths validates host values; a device tensor is used as it is (see ragged_lengths)")
    if t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"lengths must have an integer dtype, got {t.dtype}")
    if tuple(t.shape) != (B,):
        raise ValueError(f"lengths must have shape ({B},), one entry per cloud, got {tuple(t.shape)}")
    minimum = max(int(minimum), 1)
    t = t.to(torch.int64)
    bad = ((t < minimum) | (t > n_pts)).nonzero()
    if bad.numel():
        b = int(bad[0])
        raise ValueError(f"lengths[{b}] = {int(t[b])}: cloud {b} must hold between {minimum} and n_pts = {n_pts} points")
    return t.to(torch.int32).contiguous()


def ragged_lengths(lengths, B: int, n_pts: int, device, minimum: int = 1) -> torch.Tensor:
    """The (B,) int32 device tensor the ragged kernels read.  A list or a CPU tensor is validated on the host (check_lengths) and
    uploaded.  An int32 tensor already on the device is used as it is, without a synchronisation: only its dtype, shape and device are
    looked at, THE CALLER VOUCHES FOR THE RANGE minimum <= lengths[b] <= n_pts, and the kernels clamp every value into 1..n_pts, so a
    bad one cannot cause an access out of bounds -- it gives the result of the clamped length (and, below `minimum`, the repeated
    entries the kernels document for a cloud shorter than what is asked of it)."""
    device = torch.device(device)
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,):
            raise ValueError(f"a device lengths tensor must be int32 of shape ({B},), got {lengths.dtype} {tuple(lengths.shape)}")
        if lengths.device.type != device.type or (device.index is not None and lengths.device.index != device.index):
            raise ValueError(f"lengths is on {lengths.device}, the batch on {device}")
        return lengths.contiguous()
    return check_lengths(lengths, B, n_pts, minimum).to(device)


class PackedLengths(NamedTuple):
    """What the packed-row kernels of the vanilla PointNet read (packed_lengths)."""
    lens_dev: torch.Tensor      # (B,) int32 on the device
    offs_dev: torch.Tensor      # (B + 1,) int32 on the device: exclusive prefix sum of the lengths, offs[B] = M_total
    M_total: Optional[int]      # sum of the lengths (the packed row count), None when it was not asked for


def packed_offsets(lengths) -> list:
    """Host lengths -> the B + 1 exclusive prefix sums: row n of cloud b is packed row offsets[b] + n, offsets[B] the row count."""
    offs = [0]
    for v in host_lengths(lengths):
        offs.append(offs[-1] + v)
    return offs


def packed_lengths(lengths, B: int, n_pts: int, device, need_total: bool = True) -> PackedLengths:
    """lengths -> PackedLengths for a padded (B, n_pts) batch whose valid rows are stored packed, cloud after cloud.  A PackedLengths
    is passed through (so a model builds it once per forward).  A list or a CPU tensor is validated on the host (check_lengths) and
    the offsets and M_total come from the host values: no synchronisation.  An int32 tensor on the device is clamped into 1..n_pts
    and prefix-summed there by one small launch (pnpp_pn_offsets; the caller vouches for the range, as for ragged_lengths), and
    M_total COSTS ONE READ-BACK (a synchronisation): packed row counts size allocations, so a training step needs the number on the
    host.  A caller that allocates nothing by it -- the forward-only Predictor, whose buffers keep the padded shape -- passes
    need_total=False and stays free of synchronisations (and capturable)."""
    if isinstance(lengths, PackedLengths):
        if lengths.lens_dev.shape[0] != B:
            raise ValueError(f"lengths were packed for {lengths.lens_dev.shape[0]} clouds, the batch has {B}")
        if need_total and lengths.M_total is None:
            return lengths._replace(M_total=int(lengths.offs_dev[-1].item()))
        return lengths
    device = torch.device(device)
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        from . import _lib as L
        raw = ragged_lengths(lengths, B, n_pts, device)
        both = torch.empty(2 * B + 1, dtype=torch.int32, device=raw.device)
        lens, offs = both[:B], both[B:]
        with torch.cuda.device(raw.device):
            L.check(L.lib().pnpp_pn_offsets(raw.data_ptr(), B, int(n_pts), lens.data_ptr(), offs.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
        return PackedLengths(lens, offs, int(offs[-1].item()) if need_total else None)
    host = check_lengths(lengths, B, n_pts)
    offs = packed_offsets(host)
    return PackedLengths(host.to(device), torch.tensor(offs, dtype=torch.int32).to(device), offs[-1])


def host_lengths(lengths) -> list:
    """The lengths as Python ints, for the two samplers that draw on the host generator.  A device tensor is read back here (one
    synchronisation); a list or CPU tensor costs nothing."""
    if isinstance(lengths, torch.Tensor):
        return [int(v) for v in lengths.tolist()]
    return [int(v) for v in lengths]


def device_and_draw_lengths(lengths, B: int, n_pts: int, device, minimum: int, sampler: str):
    """-> (the device tensor the kernels read (ragged_lengths), what a level's centre draw should be given): the 'device' sampler draws
    from the device tensor; the two host samplers get the caller's own host values when there are any, so that only a lengths tensor
    that lives on the device alone is ever read back."""
    on_device = isinstance(lengths, torch.Tensor) and lengths.is_cuda
    dev = ragged_lengths(lengths, B, n_pts, device, minimum)
    return dev, (dev if on_device or sampler == "device" else host_lengths(lengths))


def fps_starts(lengths) -> torch.Tensor:
    """First indices of a ragged batch's farthest-point runs: torch.randint(0, lengths[b]) per cloud on the host generator, clouds in
    batch order -- the draws the per-cloud calls make (PointNet++Demo.py:20 on each cloud alone).  (B,) int64 on the CPU."""
    return torch.cat([torch.randint(0, n, (1,), dtype=torch.long) for n in host_lengths(lengths)])


def sa_minimum_length(sampler: str, grouper, npoint: int, nsample: int) -> int:
    """The shortest cloud a model's first set-abstraction level takes: a random sampler draws npoint distinct rows and kNN lists
    nsample distinct neighbours, so max(npoint, nsample) ('randperm', 'device') or nsample ('fps', which may revisit points) with kNN;
    farthest-point sampling with the radius query pads its lists and takes any cloud of at least one point.  A random sampler with
    the radius query still needs its npoint distinct rows."""
    knn = grouper == "knn"
    if sampler == "fps":
        return int(nsample) if knn else 1
    return max(int(npoint), int(nsample)) if knn else int(npoint)
