"""Host side of the HIP operators: argument checking, workspace allocation (torch caching
allocator), stream plumbing and torch.autograd glue around the C ABI of libpnpp_hip.so.

Every function here requires float32 tensors on an AMD GPU; there is no CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L
from .lengths import fps_starts, packed_lengths, ragged_lengths


# ------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------
def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on '{t.device}': the pnpp HIP operators run on an AMD GPU only "
                           "(no CPU fallback exists in this package)")


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    _need_gpu(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _i32(t: torch.Tensor, name: str) -> torch.Tensor:
    _need_gpu(t, name)
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{name} must be an integer tensor, got {t.dtype}")
    return t.to(torch.int32).contiguous()


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _nbt(bn) -> Optional[torch.Tensor]:
    """A BatchNorm's num_batches_tracked as the int64 device scalar the kernels increment (None when it is not tracked)."""
    t = getattr(bn, "num_batches_tracked", None)
    if t is None:
        return None
    _need_gpu(t, "num_batches_tracked")
    if t.dtype != torch.int64:
        raise TypeError(f"num_batches_tracked must be int64, got {t.dtype}")
    return t


def grad_sink(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The slice of an optimiser's flat gradient buffer that the backward kernels may OVERWRITE with p's gradient
    (FlatAdam(fused_grads=True)), or None when the gradient has to go through autograd's accumulation instead.

    Overwriting is only right for the first use of a parameter between two zero_grad()/step() calls.  A second use --
    gradient accumulation over micro-batches, two forward passes summed into one loss, shared weights -- gets None: its
    gradient is then returned to autograd, which ADDS it to p.grad (the same memory), so nothing is lost.  The claim is
    taken when the forward pass records the destination; FlatAdam.zero_grad()/step() release it."""
    if p is None or not torch.is_grad_enabled():
        return None
    sink = getattr(p, "_pnpp_grad_sink", None)
    if sink is None:
        return None
    if getattr(p, "_pnpp_sink_claimed", False):
        # a second use in this window: autograd will ADD its gradient to the sink's memory, possibly in the same backward pass as
        # the first use's overwrite (two passes summed into one loss) -- the overwrite must then be in place when its node returns
        p._pnpp_sink_shared = True
        return None
    p._pnpp_sink_claimed = True
    return sink


_dropout_counters = {}


def _dropout_counter(device: torch.device) -> torch.Tensor:
    """Device-side stream id of the in-kernel dropout draws: [counter, ticket word], bumped by the kernels themselves."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    c = _dropout_counters.get(key)
    if c is None:
        c = torch.zeros(2, dtype=torch.int64, device=device)
        _dropout_counters[key] = c
    return c


_scratch_cache = {}


def _scratch(nbytes: int, device: torch.device, keep_tail: bool = False) -> torch.Tensor:
    """Transient workspace, reused per (device, stream): all consumers are ordered on that stream.  A deferred reduction that still
    reads its slabs out of it (_TailSlot) is launched first, unless the caller is the level that takes it over (keep_tail)."""
    key = (device.index, _stream())
    if not keep_tail:
        slot = _tail_slots.get(key)
        if slot is not None and slot.pending is not None:
            slot.run_pending()
    buf = _scratch_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _scratch_cache[key] = buf
    return buf


def _workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    """A call's kept workspace.  The size queries answer a descriptor the library rejects with 0 bytes (and its message)."""
    if nbytes == 0:
        L.check(L.PNPP_ERR_ARG)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _bn_momentum(bn) -> float:
    return bn.momentum if bn.momentum is not None else 0.1


def _grad_dests(params, sinks):
    """Where the backward kernels write the gradients of `params` (None entries: no such parameter): a parameter's flat-buffer sink
    when an optimiser registered one (autograd then has nothing to accumulate), else a fresh tensor, allocated in the order given.
    Returns (dests, returned): the destinations, and what goes back to autograd -- None wherever a sink took the gradient."""
    dests, returned = [], []
    for p, s in zip(params, sinks or [None] * len(params)):
        fresh = torch.empty_like(p) if (p is not None and s is None) else None
        dests.append(s if s is not None else fresh)
        returned.append(fresh)
    return dests, returned


def set_matmul_precision(mode: str) -> None:
    """'f32' (default: exact float32 MFMA, the reference's arithmetic) or 'bf16' (throughput mode: the grouped layers' large
    GEMMs round their two operands to bfloat16 and accumulate in float32; everything else stays float32 / float64).
    Process-wide; a hipGraph captured under one mode keeps it."""
    if mode not in ("f32", "bf16"):
        raise ValueError(f"matmul precision must be 'f32' or 'bf16', got {mode!r}")
    L.check(L.lib().pnpp_set_matmul_precision(1 if mode == "bf16" else 0))


def get_matmul_precision() -> str:
    return "bf16" if L.lib().pnpp_get_matmul_precision() else "f32"


def set_float32_products(mode: str) -> None:
    """How the float32 products of the grouped layers' large GEMMs are formed: 'split' (default: six exact bf16 x bf16 partial products
    of three-way operand splits on the bf16 matrix pipe, float32 accumulation -- float32 results to float32 rounding, 2.67 x the
    float32 MFMA rate; csrc/gemm_wsf3_kernels.hip) or 'mfma' (v_mfma_f32_32x32x2_f32).  Process-wide; unrelated to
    set_matmul_precision, which ROUNDS operands to one bfloat16."""
    if mode not in ("split", "mfma"):
        raise ValueError(f"float32 products must be 'split' or 'mfma', got {mode!r}")
    L.check(L.lib().pnpp_set_split_products(1 if mode == "split" else 0))


def get_float32_products() -> str:
    return "split" if L.lib().pnpp_get_split_products() else "mfma"


STORE_DW_SLABS, STORE_STAT_SLABS, STORE_STREAMS = 1, 2, 4


def set_store_policy(mask: int) -> None:
    """Which classes of the large kernels' stores are write-through instead of plain write-back: a sum of STORE_DW_SLABS (dW partial
    slabs), STORE_STAT_SLABS (float64 statistics slabs) and STORE_STREAMS (streamed activation / gradient outputs).  Results do not
    depend on it (bit-identical); default STORE_DW_SLABS + STORE_STREAMS.  Process-wide; a hipGraph captured under one mask keeps it."""
    L.check(L.lib().pnpp_set_store_policy(int(mask)))


def get_store_policy() -> int:
    return L.lib().pnpp_get_store_policy()


# ------------------------------------------------------------------------------------------------
# index primitives
# ------------------------------------------------------------------------------------------------
def square_distance(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    src, dst = _f32(src, "src"), _f32(dst, "dst")
    B, S, _ = src.shape
    N = dst.shape[1]
    out = torch.empty(B, S, N, device=src.device, dtype=torch.float32)
    L.check(L.lib().pnpp_square_distance(src.data_ptr(), dst.data_ptr(), B, S, N, out.data_ptr(), _stream()))
    return out


def knn(new_xyz: torch.Tensor, xyz: torch.Tensor, k: int, lengths=None) -> torch.Tensor:
    """(B,S,k) int32 neighbour indices, ascending (distance, index).
    lengths (B,): a ragged batch -- cloud b is xyz[b, :lengths[b]], row b of the result is what the call on that slice alone returns
    (every index < lengths[b]); a list or CPU tensor is checked here (k <= lengths[b] <= N), a device int32 tensor is used as it is."""
    new_xyz, xyz = _f32(new_xyz, "new_xyz"), _f32(xyz, "xyz")
    B, S, _ = new_xyz.shape
    N = xyz.shape[1]
    idx = torch.empty(B, S, k, device=xyz.device, dtype=torch.int32)
    if lengths is not None:
        lengths = ragged_lengths(lengths, B, N, xyz.device, minimum=k)
        L.check(L.lib().pnpp_knn_ragged(new_xyz.data_ptr(), xyz.data_ptr(), B, S, N, lengths.data_ptr(), int(k), idx.data_ptr(), _stream()))
        return idx
    L.check(L.lib().pnpp_knn(new_xyz.data_ptr(), xyz.data_ptr(), B, S, N, int(k), idx.data_ptr(), _stream()))
    return idx


def estimate_normals(xyz: torch.Tensor, k: int, mode: int = L.NORMALS_NONE, ref: Optional[torch.Tensor] = None, lengths=None,
                     stride: int = 3, curvature: bool = False, neighbours: bool = False):
    """One launch: the neighbour search of knn(xyz, xyz, k, lengths) with every point as a query, the float64 covariance of each
    neighbourhood and its smallest eigenvector (include/pnpp_hip.h: pnpp_estimate_normals; pnpp_hip.normals is the user-level module).
    -> (out (B,N,stride) float32, curv (B,N) float32 or None, idx (B,N,k) int32 or None).  stride 3: the normal; stride 6: the point in
    columns 0-2, the normal in 3-5.  mode: L.NORMALS_NONE / _AWAY / _TOWARD with ref (B,3) float32, the per-cloud reference point.
    lengths (B,): a ragged batch as in knn; the rows at or beyond a cloud's length come back as zeros."""
    xyz = _f32(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"xyz must be (B, N, 3), got {tuple(xyz.shape)}")
    B, N, _ = xyz.shape
    if ref is not None:
        ref = _f32(ref, "ref")
        if tuple(ref.shape) != (B, 3):
            raise ValueError(f"ref must be ({B}, 3), one reference point per cloud, got {tuple(ref.shape)}")
    if lengths is not None:
        lengths = ragged_lengths(lengths, B, N, xyz.device, minimum=k)
    out = torch.empty(B, N, int(stride), device=xyz.device, dtype=torch.float32)
    curv = torch.empty(B, N, device=xyz.device, dtype=torch.float32) if curvature else None
    idx = torch.empty(B, N, int(k), device=xyz.device, dtype=torch.int32) if neighbours else None
    tail = (int(k), int(mode), _p(ref), out.data_ptr(), int(stride), _p(curv), _p(idx), _stream())
    if lengths is not None:
        L.check(L.lib().pnpp_estimate_normals_ragged(xyz.data_ptr(), B, N, lengths.data_ptr(), *tail))
    else:
        L.check(L.lib().pnpp_estimate_normals(xyz.data_ptr(), B, N, *tail))
    return out, curv, idx


def yaw_profile(xyz: torch.Tensor, centre: torch.Tensor, table: torch.Tensor, lengths=None, nearest: bool = False, decide=None):
    """Two launches: the self-Chamfer profile of every cloud against its own copy turned about +Y by each row (cos, sin) of `table`
    (G, 2), about centre (B, 3), and the kernel that finishes its float64 partial sums (include/pnpp_hip.h: pnpp_yaw_profile,
    pnpp_yaw_symmetry; pnpp_hip.symmetry is the user-level module).
    -> dict: distance (B,G), floor (B,), nearest_dist (B,G,N) float32 and nearest_idx (B,G,N) int32 or None; with
    decide=(tol, orders, angle_stride) -- the table then has to be the uniform grid, every order has to divide G -- also score (B,G),
    order (B,) int32, count (B,) int32 and angles (B, angle_stride).  lengths (B,): a ragged batch, rows at or beyond a cloud's length
    are never read.  No read-back: capturable once `lengths` is None or a device tensor."""
    xyz, centre, table = _f32(xyz, "xyz"), _f32(centre, "centre"), _f32(table, "table")
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"xyz must be (B, N, 3), got {tuple(xyz.shape)}")
    B, N, _ = xyz.shape
    if tuple(centre.shape) != (B, 3):
        raise ValueError(f"centre must be ({B}, 3), one centre per cloud, got {tuple(centre.shape)}")
    if table.dim() != 2 or table.shape[1] != 2:
        raise ValueError(f"table must be (G, 2) rows of (cos, sin), got {tuple(table.shape)}")
    G = table.shape[0]
    dev = xyz.device
    if lengths is not None:
        lengths = ragged_lengths(lengths, B, N, dev)
    nbytes = L.lib().pnpp_yaw_workspace_bytes(B, N, G)
    ws = _workspace(nbytes, dev)
    r = {"distance": torch.empty(B, G, device=dev, dtype=torch.float32), "floor": torch.empty(B, device=dev, dtype=torch.float32),
         "nearest_dist": torch.empty(B, G, N, device=dev, dtype=torch.float32) if nearest else None,
         "nearest_idx": torch.empty(B, G, N, device=dev, dtype=torch.int32) if nearest else None}
    tail = (centre.data_ptr(), table.data_ptr(), G, ws.data_ptr(), nbytes, _p(r["nearest_dist"]), _p(r["nearest_idx"]), _stream())
    if lengths is not None:
        L.check(L.lib().pnpp_yaw_profile_ragged(xyz.data_ptr(), B, N, lengths.data_ptr(), *tail))
    else:
        L.check(L.lib().pnpp_yaw_profile(xyz.data_ptr(), B, N, *tail))
    tol, orders, n_orders, stride = 0.0, None, 0, 0
    if decide is not None:
        tol, order_list, stride = float(decide[0]), [int(m) for m in decide[1]], int(decide[2])
        n_orders = len(order_list)
        orders = (C.c_int32 * max(n_orders, 1))(*order_list)
        r["score"] = torch.empty(B, G, device=dev, dtype=torch.float32)
        r["order"] = torch.empty(B, device=dev, dtype=torch.int32)
        r["count"] = torch.empty(B, device=dev, dtype=torch.int32)
        r["angles"] = torch.empty(B, stride, device=dev, dtype=torch.float32)
    L.check(L.lib().pnpp_yaw_symmetry(ws.data_ptr(), nbytes, B, N, _p(lengths), G, tol, orders, n_orders, r["distance"].data_ptr(),
                                      r["floor"].data_ptr(), _p(r.get("score")), _p(r.get("order")), _p(r.get("count")),
                                      _p(r.get("angles")), stride, _stream()))
    return r


def farthest_point_sample(xyz: torch.Tensor, npoint: int, start: Optional[torch.Tensor] = None, lengths=None) -> torch.Tensor:
    """lengths (B,): a ragged batch -- row b is the sampling of xyz[b, :lengths[b]] alone (npoint may exceed a length, as it may
    exceed N); start[b] < lengths[b].  Without `start` the first index of cloud b is torch.randint(0, lengths[b]) on the host
    generator, cloud after cloud -- the draws of the per-cloud calls in batch order; that needs the lengths on the host, so a device
    `lengths` is read back once (inject `start` to avoid it)."""
    xyz = _f32(xyz, "xyz")
    B, N, _ = xyz.shape
    if lengths is not None:
        dev_lengths = ragged_lengths(lengths, B, N, xyz.device)
        if start is None:
            start = fps_starts(lengths)
        start = start.to(device=xyz.device, dtype=torch.int32).contiguous()
        out = torch.empty(B, npoint, device=xyz.device, dtype=torch.int32)
        L.check(L.lib().pnpp_fps_ragged(xyz.data_ptr(), B, N, dev_lengths.data_ptr(), int(npoint), start.data_ptr(), out.data_ptr(),
                                        _stream()))
        return out
    if start is None:  # PointNet++Demo.py:20 draws the first index with torch.randint
        start = torch.randint(0, N, (B,), dtype=torch.long)
    start = start.to(device=xyz.device, dtype=torch.int32).contiguous()
    out = torch.empty(B, npoint, device=xyz.device, dtype=torch.int32)
    L.check(L.lib().pnpp_fps(xyz.data_ptr(), B, N, int(npoint), start.data_ptr(), out.data_ptr(), _stream()))
    return out


def ball_query(radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor, lengths=None) -> torch.Tensor:
    """lengths (B,): a ragged batch -- row b lists members of xyz[b, :lengths[b]] only, as the call on that slice alone does.
    The threshold is the reference's (PointNet++Demo.py:65, `sqrdists > radius ** 2`): the python float squared in double, rounded to
    float32 once -- by the C float parameter of the _r2 entries.  (A float32 radius squared afterwards is a different number.)"""
    xyz, new_xyz = _f32(xyz, "xyz"), _f32(new_xyz, "new_xyz")
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    r2 = float(radius) ** 2
    idx = torch.empty(B, S, nsample, device=xyz.device, dtype=torch.int32)
    if lengths is not None:
        lengths = ragged_lengths(lengths, B, N, xyz.device)
        L.check(L.lib().pnpp_ball_query_r2_ragged(new_xyz.data_ptr(), xyz.data_ptr(), B, S, N, lengths.data_ptr(), r2,
                                                  int(nsample), idx.data_ptr(), _stream()))
        return idx
    L.check(L.lib().pnpp_ball_query_r2(new_xyz.data_ptr(), xyz.data_ptr(), B, S, N, r2, int(nsample), idx.data_ptr(), _stream()))
    return idx


def sample_random(seed: int, stream_id: int, B: int, N: int, npoint: int, device, lengths=None) -> torch.Tensor:
    """lengths (B,): a ragged batch -- row b is drawn from cloud b's first lengths[b] rows, bit-equal to row b of the uniform draw
    at N = lengths[b] (a list or CPU tensor is checked here: npoint <= lengths[b] <= N)."""
    out = torch.empty(B, npoint, device=device, dtype=torch.int32)
    if lengths is not None:
        lengths = ragged_lengths(lengths, B, N, device, minimum=npoint)
        L.check(L.lib().pnpp_sample_random_ragged(int(seed) & (2**64 - 1), int(stream_id) & (2**64 - 1), B, N, lengths.data_ptr(),
                                                  int(npoint), out.data_ptr(), _stream()))
        return out
    L.check(L.lib().pnpp_sample_random(int(seed) & (2**64 - 1), int(stream_id) & (2**64 - 1), B, N, int(npoint),
                                       out.data_ptr(), _stream()))
    return out


def sample_random_dev(seed: int, counter: torch.Tensor, offset: int, B: int, N: int, npoint: int, lengths=None) -> torch.Tensor:
    """Like sample_random, with stream id = counter[0] + offset read at kernel time; the kernel then adds 1 to
    counter[0].  `counter` is an int64 device tensor of two words (call counter, ticket word kept at zero)."""
    _need_gpu(counter, "counter")
    if counter.dtype != torch.int64 or counter.numel() != 2 or not counter.is_contiguous():
        raise ValueError("counter must be a contiguous int64 tensor of 2 elements")
    out = torch.empty(B, npoint, device=counter.device, dtype=torch.int32)
    if lengths is not None:
        lengths = ragged_lengths(lengths, B, N, counter.device, minimum=npoint)
        L.check(L.lib().pnpp_sample_random_dev_ragged(int(seed) & (2**64 - 1), counter.data_ptr(), int(offset) & (2**64 - 1), B, N,
                                                      lengths.data_ptr(), int(npoint), out.data_ptr(), _stream()))
        return out
    L.check(L.lib().pnpp_sample_random_dev(int(seed) & (2**64 - 1), counter.data_ptr(), int(offset) & (2**64 - 1), B, N,
                                           int(npoint), out.data_ptr(), _stream()))
    return out


def sample_random_dev2(seed: int, counter: torch.Tensor, offset: int, B: int, N1: int, npoint1: int, N2: int, npoint2: int,
                       lengths=None):
    """Two consecutive sample_random_dev draws in one launch: (B,npoint1) from N1 with the counter's value, (B,npoint2)
    from N2 with the next one; counter[0] += 2.  Bit-identical to the two separate calls.  lengths (B,) belong to the first draw
    (the second ranks the first level's centres, which are uniform)."""
    _need_gpu(counter, "counter")
    if counter.dtype != torch.int64 or counter.numel() != 2 or not counter.is_contiguous():
        raise ValueError("counter must be a contiguous int64 tensor of 2 elements")
    out1 = torch.empty(B, npoint1, device=counter.device, dtype=torch.int32)
    out2 = torch.empty(B, npoint2, device=counter.device, dtype=torch.int32)
    if lengths is not None:
        lengths = ragged_lengths(lengths, B, N1, counter.device, minimum=npoint1)
        L.check(L.lib().pnpp_sample_random_dev2_ragged(int(seed) & (2**64 - 1), counter.data_ptr(), int(offset) & (2**64 - 1), B, N1,
                                                       lengths.data_ptr(), int(npoint1), out1.data_ptr(), N2, int(npoint2),
                                                       out2.data_ptr(), _stream()))
        return out1, out2
    L.check(L.lib().pnpp_sample_random_dev2(int(seed) & (2**64 - 1), counter.data_ptr(), int(offset) & (2**64 - 1), B, N1,
                                            int(npoint1), out1.data_ptr(), N2, int(npoint2), out2.data_ptr(), _stream()))
    return out1, out2


def subsample_points(seed: int, stream_id: int, bank: torch.Tensor, lengths: torch.Tensor, num: int,
                     cloud_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`num` points of each selected cloud of a device-resident bank (n_clouds,Lmax,3): without replacement where the
    cloud has at least `num` points, with replacement otherwise (dataloader_*: sample_pts).  Returns (B,num,3)."""
    bank = _f32(bank, "bank")
    _need_gpu(lengths, "lengths")
    if bank.dim() != 3 or bank.shape[2] != 3 or lengths.dtype != torch.int32 or lengths.numel() != bank.shape[0]:
        raise ValueError("subsample_points: bank must be (n_clouds,Lmax,3) float32 and lengths (n_clouds,) int32")
    lengths = lengths.contiguous()
    if cloud_ids is not None:
        _need_gpu(cloud_ids, "cloud_ids")
        cloud_ids = cloud_ids.to(torch.int32).contiguous()
        if cloud_ids.numel() and (int(cloud_ids.min()) < 0 or int(cloud_ids.max()) >= bank.shape[0]):
            raise IndexError("subsample_points: cloud id out of range")
    B = bank.shape[0] if cloud_ids is None else cloud_ids.numel()
    out = torch.empty(B, int(num), 3, device=bank.device, dtype=torch.float32)
    L.check(L.lib().pnpp_subsample_points(int(seed) & (2**64 - 1), int(stream_id) & (2**64 - 1), bank.data_ptr(),
                                          lengths.data_ptr(), _p(cloud_ids), B, bank.shape[1], int(num), out.data_ptr(),
                                          _stream()))
    return out


AUGMENT_KINDS = ("angle", "vm", "axis", "dir8", "keep")


def augment_plan(xyz_shape, targets, kinds, counts=None, scale=None, jitter=None):
    """Host-side validation of an augment_clouds call, from shapes alone (runs without a GPU): -> one entry per target, None for
    "keep" and (kind code, rows, cols, output shape, counts tensor or None) otherwise.  Mismatches raise ValueError."""
    if len(xyz_shape) != 3 or xyz_shape[2] not in (3, 6) or xyz_shape[0] < 1 or xyz_shape[1] < 1:
        raise ValueError(f"augment_clouds: xyz must be (B, N, 3) or (B, N, 6) with B, N >= 1, got {tuple(xyz_shape)}")
    B = xyz_shape[0]
    targets, kinds = list(targets), list(kinds)
    if len(targets) != len(kinds):
        raise ValueError(f"augment_clouds: {len(targets)} targets but {len(kinds)} kinds")
    if isinstance(counts, torch.Tensor) or counts is None:
        counts = [counts if k in ("angle", "vm") and t.dim() > (1 if k == "angle" else 2) else None for t, k in zip(targets, kinds)]
    counts = list(counts)
    if len(counts) != len(targets):
        raise ValueError(f"augment_clouds: {len(targets)} targets but {len(counts)} counts entries")
    plan = []
    for i, (t, k, cnt) in enumerate(zip(targets, kinds, counts)):
        if k not in AUGMENT_KINDS:
            raise ValueError(f"augment_clouds: target {i} has unknown kind {k!r}; kinds are {AUGMENT_KINDS}")
        if k == "keep":
            plan.append(None)
            continue
        shp = tuple(t.shape)
        if not shp or shp[0] != B:
            raise ValueError(f"augment_clouds: target {i} ({k}) has shape {shp}, the batch has {B} clouds")
        if t.dtype != torch.float32:
            raise ValueError(f"augment_clouds: target {i} ({k}) must be float32, got {t.dtype}")
        if k == "angle" and len(shp) in (1, 2):
            code, rows, cols, out = L.AUG_ANGLE, (shp[1] if len(shp) == 2 else 1), 1, shp
        elif k == "vm" and ((len(shp) == 2 and shp[1] == 2) or (len(shp) == 3 and shp[2] in (2, 3))):
            code, rows, cols, out = L.AUG_VM, (shp[1] if len(shp) == 3 else 1), shp[-1], shp
        elif k == "axis" and len(shp) in (2, 3) and shp[-1] == 3:
            code, rows, cols, out = L.AUG_AXIS, (shp[1] if len(shp) == 3 else 1), 3, shp
        elif k == "dir8" and shp == (B, 3):
            code, rows, cols, out = L.AUG_DIR8, 1, 3, (B, 8)
        else:
            raise ValueError(f"augment_clouds: target {i} of kind {k!r} cannot have shape {shp}")
        if rows < 1:
            raise ValueError(f"augment_clouds: target {i} ({k}) has no rows")
        if cnt is not None and (tuple(cnt.shape) != (B,) or cnt.dtype not in (torch.int32, torch.int64)):
            raise ValueError(f"augment_clouds: counts of target {i} must be an integer tensor of shape ({B},)")
        plan.append((code, rows, cols, out, cnt))
    if sum(p is not None for p in plan) > L.PNPP_AUG_MAX_TARGETS:
        raise ValueError(f"augment_clouds: at most {L.PNPP_AUG_MAX_TARGETS} transformed targets per launch")
    if scale is not None:
        lo, hi = (float(v) for v in scale)
        if not (0.0 < lo <= hi < float("inf")):
            raise ValueError(f"augment_clouds: scale=(lo, hi) needs 0 < lo <= hi, got {scale}")
    if jitter is not None:
        sigma, clip = (float(v) for v in jitter)
        if not (0.0 <= sigma < float("inf") and clip >= 0.0):
            raise ValueError(f"augment_clouds: jitter=(sigma, clip) needs sigma >= 0 and clip >= 0, got {jitter}")
    return plan


def augment_clouds(xyz: torch.Tensor, seed: int, stream_id: int, targets=(), kinds=(), counts=None, lengths=None, yaw: bool = True,
                   scale=None, jitter=None, dirs8: Optional[torch.Tensor] = None):
    """A batch in a new pose, targets moved along, in one launch (pnpp_augment_clouds): -> (xyz', [targets'], params).

    xyz (B,N,3) or (B,N,6) float32; cloud b is turned by theta_b about +Y (yaw), scaled by a factor from scale=(lo, hi) and
    jittered per point with jitter=(sigma, clip) -- each only when asked for, out of place.  kinds[i] says what targets[i] is:
    "angle" (B,) / (B,k): mu - theta wrapped into (-pi, pi]; "vm" (B,2) / (B,K,2) / (B,K,3): column 0 as angle; "axis" (B,3) /
    (B,k,3): rotated; "dir8" (B,3) forward axis -> (B,8) soft labels over dirs8 (8,3); "keep": returned as it is.  counts: per
    target (or one tensor for every multi-row angle / vm target) the (B,) number of leading rows that are real.  lengths (B,):
    rows at or beyond lengths[b] are copied.  params (B,4) = [cos, sin, scale, theta].  A pure function of (seed, stream_id)."""
    plan = augment_plan(xyz.shape, targets, kinds, counts, scale, jitter)
    xyz = _f32(xyz, "xyz")
    B, N, Cc = xyz.shape
    d = L.AugmentDesc()
    d.flags = (L.AUG_YAW if yaw else 0) | (L.AUG_SCALE if scale is not None else 0) | (L.AUG_JITTER if jitter is not None else 0)
    if scale is not None:
        d.scale_lo, d.scale_hi = float(scale[0]), float(scale[1])
    if jitter is not None:
        d.sigma, d.clip = float(jitter[0]), float(jitter[1])
    outs = []
    held = []   # converted copies (contiguous, int32) must stay allocated until the launch that reads them is enqueued
    n = 0
    for t, p in zip(targets, plan):
        if p is None:
            outs.append(t)
            continue
        code, rows, cols, out_shape, cnt = p
        tin = _f32(t, "target")
        tout = torch.empty(out_shape, device=xyz.device, dtype=torch.float32)
        g = d.targets[n]
        g.kind, g.rows, g.cols, g.inp, g.out = code, rows, cols, tin.data_ptr(), tout.data_ptr()
        if cnt is not None:
            cnt = _i32(cnt, "counts")
            g.counts = cnt.data_ptr()
        if code == L.AUG_DIR8:
            if dirs8 is None or tuple(dirs8.shape) != (8, 3):
                raise ValueError("augment_clouds: a dir8 target needs dirs8 of shape (8, 3)")
            dirs8 = _f32(dirs8, "dirs8")
            d.dirs8 = dirs8.data_ptr()
        held += [tin, cnt]
        outs.append(tout)
        n += 1
    d.n_targets = n
    if lengths is not None:
        if not isinstance(lengths, torch.Tensor) or tuple(lengths.shape) != (B,):
            raise ValueError(f"augment_clouds: lengths must be a tensor of shape ({B},)")
        lengths = _i32(lengths, "lengths")
    out = torch.empty_like(xyz)
    params = torch.empty(B, 4, device=xyz.device, dtype=torch.float32)
    L.check(L.lib().pnpp_augment_clouds(int(seed) & (2**64 - 1), int(stream_id) & (2**64 - 1), xyz.data_ptr(), out.data_ptr(), _p(lengths),
                                        B, N, Cc, C.byref(d), params.data_ptr(), _stream()))
    return out, outs, params


VIEW_ELEVATION = (-0.5235987755982988, 1.0471975511965976)   # (-pi/6, pi/3): from slightly below to well above


def view_resolution(N: int) -> int:
    """The default depth-buffer side for clouds of N rows: about one point per cell, at most the kernel's 128."""
    import math
    return min(L.VIEW_MAX_G, max(1, math.isqrt(max(int(N), 1) - 1) + 1))


def view_plan(xyz_shape, resolution=None, splat: int = 1, thickness: float = 0.1, elevation=VIEW_ELEVATION, drop: float = 0.0,
              min_keep: int = 1, lengths=None, view_dirs=None, angles=None):
    """Host-side validation of a view_clouds call, from shapes and numbers alone (runs without a GPU): -> (G, splat, thickness,
    (lo, hi), drop, min_keep, flags).  What pnpp_view_clouds would refuse raises ValueError here, before anything is counted."""
    import math
    if len(xyz_shape) != 3 or xyz_shape[2] not in (3, 6):
        raise ValueError(f"view_clouds: xyz must be (B, N, 3) or (B, N, 6), got {tuple(xyz_shape)}")
    B, N = int(xyz_shape[0]), int(xyz_shape[1])
    if not 1 <= B <= 65535 or not 1 <= N <= 1 << 24:
        raise ValueError(f"view_clouds: B must be 1..65535 and N 1..2^24, got B={B} N={N}")
    G = view_resolution(N) if resolution is None else int(resolution)
    if not 1 <= G <= L.VIEW_MAX_G:
        raise ValueError(f"view_clouds: resolution={resolution} must be 1..{L.VIEW_MAX_G}")
    if int(splat) != splat or not 0 <= int(splat) <= 2:
        raise ValueError(f"view_clouds: splat={splat} must be 0, 1 or 2")
    thickness = float(thickness)
    if not 0.0 <= thickness < float("inf"):
        raise ValueError(f"view_clouds: thickness={thickness} must be finite and >= 0")
    try:
        lo, hi = (float(v) for v in elevation)
    except (TypeError, ValueError):
        raise ValueError(f"view_clouds: elevation must be a (lo, hi) pair, got {elevation!r}") from None
    if not -math.pi / 2 <= lo <= hi <= math.pi / 2:
        raise ValueError(f"view_clouds: elevation=(lo, hi) needs -pi/2 <= lo <= hi <= pi/2, got {elevation}")
    drop = float(drop)
    if not 0.0 <= drop < 1.0:
        raise ValueError(f"view_clouds: drop={drop} must be in [0, 1)")
    if int(min_keep) != min_keep or not 0 <= int(min_keep) <= N:
        raise ValueError(f"view_clouds: min_keep={min_keep} must be 0..N={N}")
    if lengths is not None and (not isinstance(lengths, torch.Tensor) or tuple(lengths.shape) != (B,)
                                or lengths.dtype not in (torch.int32, torch.int64)):
        raise ValueError(f"view_clouds: lengths must be an integer tensor of shape ({B},)")
    if view_dirs is not None and angles is not None:
        raise ValueError("view_clouds: view_dirs or angles, not both")
    flags = 0
    for t, cols, flag, name in ((view_dirs, 3, L.VIEW_DIRS, "view_dirs"), (angles, 2, L.VIEW_ANGLES, "angles")):
        if t is not None:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, cols) or t.dtype != torch.float32:
                raise ValueError(f"view_clouds: {name} must be a float32 tensor of shape ({B}, {cols})")
            flags = flag
    return G, int(splat), thickness, (lo, hi), drop, int(min_keep), flags


def view_clouds(xyz: torch.Tensor, seed: int, stream_id: int, lengths=None, resolution=None, splat: int = 1, thickness: float = 0.1,
                elevation=VIEW_ELEVATION, drop: float = 0.0, min_keep: int = 1, view_dirs=None, angles=None, index: bool = False):
    """What one viewer at infinity sees of each cloud, in one launch (pnpp_view_clouds): -> (xyz', lengths', params[, index]).

    xyz (B,N,3) or (B,N,6) float32, lengths (B,) or None.  Cloud b is seen from a direction drawn per cloud (azimuth uniform about
    +Y, elevation uniform in `elevation`), or from view_dirs (B,3) -- towards the viewer -- or angles (B,2) = [azimuth, elevation].  A
    depth buffer of resolution^2 cells over the view plane (None: about one point per cell) keeps, per cell and its `splat`
    neighbours, the depth nearest the viewer; a point survives when it lies within thickness x extent of it, and then with the
    cloud's own probability 1 - ratio, ratio uniform in [0, drop).  xyz' holds the survivors in their input order followed by exact
    zeros, lengths' (B,) int32 their number; a cloud left with fewer than min_keep passes through whole.  params (B,8) = [v_x, v_y,
    v_z, azimuth, elevation, cell, kept, passed_through]; index (B,N) int32: the source row of each output row, -1 in the padding.
    A pure function of (seed, stream_id); nothing is read back."""
    G, splat, thickness, (lo, hi), drop, min_keep, flags = view_plan(xyz.shape, resolution, splat, thickness, elevation, drop, min_keep,
                                                                     lengths, view_dirs, angles)
    xyz = _f32(xyz, "xyz")
    B, N, Cc = xyz.shape
    d = L.ViewDesc()
    d.G, d.splat, d.thickness, d.elev_lo, d.elev_hi, d.drop, d.min_keep, d.flags = G, splat, thickness, lo, hi, drop, min_keep, flags
    given = view_dirs if view_dirs is not None else angles
    if given is not None:
        given = _f32(given, "view_dirs")   # held until the launch is enqueued
        d.view_dirs = given.data_ptr()
    if lengths is not None:
        lengths = _i32(lengths, "lengths")
    out = torch.empty_like(xyz)
    lengths_out = torch.empty(B, device=xyz.device, dtype=torch.int32)
    params = torch.empty(B, 8, device=xyz.device, dtype=torch.float32)
    idx = torch.empty(B, N, device=xyz.device, dtype=torch.int32) if index else None
    L.check(L.lib().pnpp_view_clouds(int(seed) & (2**64 - 1), int(stream_id) & (2**64 - 1), xyz.data_ptr(), out.data_ptr(), _p(lengths),
                                     lengths_out.data_ptr(), _p(idx), B, N, Cc, C.byref(d), params.data_ptr(), _stream()))
    return (out, lengths_out, params, idx) if index else (out, lengths_out, params)


SCAN_CENTRES = {None: L.SCAN_NONE, "centroid": L.SCAN_CENTROID, "box": L.SCAN_BOX}
SCAN_SCALES = {None: L.SCAN_NONE, "sphere": L.SCAN_SPHERE, "box": L.SCAN_BOX}
_SCAN_UNSET = object()


def scan_plan(xyz_shape, cell=None, grid=None, k=None, std_ratio=2.0, centre=_SCAN_UNSET, scale=_SCAN_UNSET, lengths=None):
    """Host-side validation of the raw-scan steps, from shapes and numbers alone (runs without a GPU): what pnpp_voxel_downsample
    (cell or grid given), pnpp_outlier_statistic / _filter (k given) and pnpp_normalize_clouds (centre or scale given) would refuse
    raises ValueError here, in the entry's own words.  -> dict of the checked values (cell, grid, k, std_ratio, centre, scale codes)."""
    if len(xyz_shape) != 3 or xyz_shape[2] not in (3, 6):
        raise ValueError(f"scan: xyz must be (B, N, 3) or (B, N, 6), got {tuple(xyz_shape)}")
    B, N = int(xyz_shape[0]), int(xyz_shape[1])
    if not 1 <= B <= 65535 or not 1 <= N <= 1 << 24:
        raise ValueError(f"scan: B must be 1..65535 and N 1..2^24, got B={B} N={N}")
    if lengths is not None and (not isinstance(lengths, torch.Tensor) or tuple(lengths.shape) != (B,)
                                or lengths.dtype not in (torch.int32, torch.int64)):
        raise ValueError(f"scan: lengths must be an integer tensor of shape ({B},)")
    plan = {}
    if cell is not None or grid is not None:
        if cell is not None and grid is not None:
            raise ValueError(f"voxel_downsample: exactly one of cell and grid is given, got cell={cell} grid={grid}")
        if cell is not None:
            cell = float(cell)
            if not 0.0 < cell < float("inf"):
                raise ValueError(f"voxel_downsample: cell={cell} must be finite and > 0")
        else:
            if int(grid) != grid or not 1 <= int(grid) <= L.VOXEL_MAX_GRID:
                raise ValueError(f"voxel_downsample: grid={grid} must be 1..{L.VOXEL_MAX_GRID}")
            grid = int(grid)
        plan["cell"], plan["grid"] = cell, grid
    if k is not None:
        if int(k) != k or not 1 <= int(k) <= L.OUTLIER_MAX_K:
            raise ValueError(f"remove_outliers: k={k} must be 1..{L.OUTLIER_MAX_K}")
        if lengths is None and N < int(k) + 1:
            raise ValueError(f"remove_outliers: clouds of N={N} rows have no k + 1 = {int(k) + 1} neighbours to list")
        std_ratio = float(std_ratio)
        if not 0.0 <= std_ratio < float("inf"):
            raise ValueError(f"remove_outliers: std_ratio={std_ratio} must be finite and >= 0")
        plan["k"], plan["std_ratio"] = int(k), std_ratio
    if centre is not _SCAN_UNSET or scale is not _SCAN_UNSET:
        centre = None if centre is _SCAN_UNSET else centre
        scale = None if scale is _SCAN_UNSET else scale
        if centre not in SCAN_CENTRES:
            raise ValueError(f"normalize_clouds: centre={centre!r} must be 'centroid', 'box' or None")
        if scale not in SCAN_SCALES:
            raise ValueError(f"normalize_clouds: scale={scale!r} must be 'sphere', 'box' or None")
        plan["centre"], plan["scale"] = SCAN_CENTRES[centre], SCAN_SCALES[scale]
    return plan


def _scan_outputs(xyz: torch.Tensor, index: bool):
    B, N, _ = xyz.shape
    return (torch.empty_like(xyz), torch.empty(B, device=xyz.device, dtype=torch.int32),
            torch.empty(B, N, device=xyz.device, dtype=torch.int32) if index else None)


def voxel_downsample(xyz: torch.Tensor, cell=None, grid=None, lengths=None, index: bool = False):
    """One point per occupied cell of a per-cloud grid (pnpp_voxel_downsample): -> (xyz', lengths'[, index]).

    xyz (B,N,3) or (B,N,6) float32, lengths (B,) or None.  `cell` is the cells' edge; `grid` instead the number of cells along the
    cloud's longest axis (1..1024).  The grid starts at the cloud's lower corner and has ten bits per axis: cells beyond index 1023
    merge into the last; with `grid` the last index is grid - 1, so the cloud's far face belongs to the last cell and grid=1 keeps
    one point.  A cell's survivor is the point nearest its centre (the lowest row among equals) -- a real point with its
    own normal and source row, where Open3D and PCL return the cell's centroid.  Survivors keep their input order, exact zeros
    follow, lengths' (B,) int32 counts them, index (B,N) int32 is the source row of each output row (-1 in the padding).  Integer
    atomics only: two calls give the same bits; nothing is read back."""
    plan = scan_plan(xyz.shape, cell=cell, grid=grid, lengths=lengths)
    if "grid" not in plan:
        raise ValueError("voxel_downsample: exactly one of cell and grid is given, got neither")
    xyz = _f32(xyz, "xyz")
    B, N, Cc = xyz.shape
    if lengths is not None:
        lengths = _i32(lengths, "lengths")
    nbytes = L.lib().pnpp_voxel_workspace_bytes(B, N)
    ws = _workspace(nbytes, xyz.device)
    out, lengths_out, idx = _scan_outputs(xyz, index)
    L.check(L.lib().pnpp_voxel_downsample(xyz.data_ptr(), out.data_ptr(), _p(lengths), lengths_out.data_ptr(), _p(idx), B, N, Cc,
                                          plan["cell"] or 0.0, plan["grid"] or 0, ws.data_ptr(), nbytes, _stream()))
    return (out, lengths_out, idx) if index else (out, lengths_out)


def outlier_statistic(xyz: torch.Tensor, lists: torch.Tensor, lengths=None) -> torch.Tensor:
    """(B,N) float64: per point the mean distance to its k listed neighbours, lists (B,N,k+1) int32 (pnpp_outlier_statistic)."""
    xyz = _f32(xyz, "xyz")
    B, N, Cc = xyz.shape
    if lists.dim() != 3 or tuple(lists.shape[:2]) != (B, N) or lists.dtype != torch.int32 or lists.shape[2] < 2:
        raise ValueError(f"outlier_statistic: lists must be int32 of shape ({B}, {N}, k + 1), got {lists.dtype} {tuple(lists.shape)}")
    _need_gpu(lists, "lists")
    lists = lists.contiguous()
    if lengths is not None:
        lengths = _i32(lengths, "lengths")
    stat = torch.empty(B, N, device=xyz.device, dtype=torch.float64)
    L.check(L.lib().pnpp_outlier_statistic(xyz.data_ptr(), lists.data_ptr(), _p(lengths), B, N, Cc, lists.shape[2] - 1, stat.data_ptr(),
                                           _stream()))
    return stat


def remove_outliers(xyz: torch.Tensor, k: int = 16, std_ratio: float = 2.0, lengths=None, index: bool = False, stats: bool = False):
    """Statistical outlier removal as PCL and Open3D define it: -> (xyz', lengths'[, index][, stats]).

    Per point the mean distance s to its k nearest neighbours (ops.knn of the cloud on itself with k + 1: the search is brute force,
    O(N^2) per cloud, so on a large scan this step belongs after voxel_downsample); per cloud the mean and population standard
    deviation of s in float64; a point is kept when s <= mean + std_ratio std.  A cloud with no more than k points passes through
    whole (decided on the device).  The mean / std rule is not robust: a heavy contamination raises its own threshold.  Output as
    voxel_downsample's; stats (B,4) float64 = [mean, std, thr, kept] stays on the device."""
    plan = scan_plan(xyz.shape, k=k, std_ratio=std_ratio, lengths=lengths)
    xyz = _f32(xyz, "xyz")
    B, N, Cc = xyz.shape
    if lengths is not None:
        lengths = _i32(lengths, "lengths")   # a device tensor: short clouds are the filter kernel's business, not the search's
    pts = xyz if Cc == 3 else xyz[..., :3].contiguous()
    kk = min(plan["k"] + 1, N)   # a ragged batch padded to fewer than k + 1 rows: every cloud passes through, the lists are never read
    lists = knn(pts, pts, kk, lengths)
    if kk < plan["k"] + 1:
        lists = lists.new_zeros(B, N, plan["k"] + 1)
    stat = outlier_statistic(xyz, lists, lengths)
    out, lengths_out, idx = _scan_outputs(xyz, index)
    st = torch.empty(B, 4, device=xyz.device, dtype=torch.float64) if stats else None
    L.check(L.lib().pnpp_outlier_filter(xyz.data_ptr(), out.data_ptr(), stat.data_ptr(), _p(lengths), lengths_out.data_ptr(), _p(idx),
                                        _p(st), B, N, Cc, plan["k"], plan["std_ratio"], _stream()))
    return (out, lengths_out) + ((idx,) if index else ()) + ((st,) if stats else ())


def normalize_clouds(xyz: torch.Tensor, lengths=None, centre="centroid", scale="sphere"):
    """Every cloud in its own unit frame, one launch (pnpp_normalize_clouds): -> (xyz', centre (B,3), scale (B,)).

    centre: "centroid" (the float64 mean of the valid rows, rounded to float32), "box" (the middle of the bounding box) or None;
    scale: "sphere" (the largest distance from the centre), "box" (half the longest box edge) or None; a scale of 0 becomes 1.
    x' = (x - centre) / scale; columns 3..5 are unchanged, padding rows come back as zeros.  centre and scale map a result back."""
    plan = scan_plan(xyz.shape, centre=centre, scale=scale, lengths=lengths)
    xyz = _f32(xyz, "xyz")
    B, N, Cc = xyz.shape
    if lengths is not None:
        lengths = _i32(lengths, "lengths")
    out = torch.empty_like(xyz)
    c = torch.empty(B, 3, device=xyz.device, dtype=torch.float32)
    r = torch.empty(B, device=xyz.device, dtype=torch.float32)
    L.check(L.lib().pnpp_normalize_clouds(xyz.data_ptr(), out.data_ptr(), _p(lengths), B, N, Cc, plan["centre"], plan["scale"],
                                          c.data_ptr(), r.data_ptr(), _stream()))
    return out, c, r


class _IndexPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx):
        points = _f32(points, "points")
        idx32 = _i32(idx, "idx")
        B, N, Cc = points.shape
        M = idx32[0].numel()
        out = torch.empty(*idx32.shape, Cc, device=points.device, dtype=torch.float32)
        L.check(L.lib().pnpp_index_points(points.data_ptr(), idx32.data_ptr(), B, N, Cc, M, out.data_ptr(), _stream()))
        ctx.save_for_backward(idx32)
        ctx.shape = (B, N, Cc, M)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx32,) = ctx.saved_tensors
        B, N, Cc, M = ctx.shape
        dout = _f32(dout, "dout")
        dpoints = torch.zeros(B, N, Cc, device=dout.device, dtype=torch.float32)
        L.check(L.lib().pnpp_index_points_bwd(dout.data_ptr(), idx32.data_ptr(), B, N, Cc, M, dpoints.data_ptr(), _stream()))
        return dpoints, None


def index_points(points: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    return _IndexPoints.apply(points, idx)


# ------------------------------------------------------------------------------------------------
# set abstraction
# ------------------------------------------------------------------------------------------------
def _sa_desc(B, N, S, K, D, channels: Sequence[int], group_all: bool, training: bool, eps: float, momentum: float):
    d = L.SaDesc()
    d.B, d.N, d.S, d.K, d.D, d.L = B, N, S, K, D, len(channels)
    for i, c in enumerate(channels):
        d.C[i] = int(c)
    d.group_all, d.training = int(group_all), int(training)
    d.eps, d.momentum = float(eps), float(momentum)
    return d


def _ptr_array(tensors: Sequence[Optional[torch.Tensor]]):
    arr = (C.c_void_p * L.PNPP_MAX_LAYERS)()
    for i, t in enumerate(tensors):
        arr[i] = _p(t)
    return arr


# ---- a level's trailing dW reduction rides in the next level's pooling launch (pnpp_sa_backward_ex) ----
# PNPP_RIDE_TAILS=0 (read once): every level launches its own reductions, as pnpp_sa_backward does -- the A/B switch
_RIDE_TAILS = os.environ.get("PNPP_RIDE_TAILS", "1") != "0"


class _TailSlot:
    """What one (device, stream) carries from one set-abstraction backward call to the next inside a backward pass.

    pending: the deferred reduction of the level that ran last (L.SaTail), with `keep` -- the scratch buffer it reads and the
    gradient buffer it writes -- held until it has run.  The next level's call takes it as `ride`; whatever is still pending when
    the engine finishes the pass (the lower level frozen, the graph cut between the levels, one level alone) is launched by the
    callback registered on the pass's first deferral.  The levels share the stream's scratch buffer: the level that takes a tail
    over checks its own layout against the slabs the tail reads (pnpp_sa_backward_ex); any other user of the buffer runs the tail
    first (_scratch)."""

    def __init__(self):
        self.task = -1          # the backward pass (graph task id) whose end-of-pass callback is registered
        self.pending = None     # (L.SaTail, stream handle, torch stream, keep)

    def take(self):
        t, self.pending = self.pending, None
        return t

    def flush(self) -> None:   # the end of the pass
        self.task = -1
        self.run_pending()

    def run_pending(self) -> None:
        t = self.take()
        if t is None:
            return
        tail, stream, tstream, _keep = t
        L.check(L.lib().pnpp_sa_run_tail(C.byref(tail), stream))
        cur = torch.cuda.current_stream(tstream.device)
        if cur != tstream:   # the pass ran on another stream than the one its caller goes on with
            cur.wait_stream(tstream)


_tail_slots = {}


def _tail_slot(device: torch.device):
    """The slot to defer into, or None where nothing may be deferred: riding switched off, or no backward pass of the autograd
    engine around this call whose end would flush it (a direct call of backward(), a custom driver)."""
    if not _RIDE_TAILS or not hasattr(torch._C, "_current_graph_task_id"):
        return None
    task = torch._C._current_graph_task_id()
    if task < 0:
        return None
    key = (device.index, _stream())
    slot = _tail_slots.get(key)
    if slot is None:
        slot = _tail_slots[key] = _TailSlot()
    if slot.task != task:
        slot.run_pending()   # left by a pass that ended without its callback (an exception between two levels): never lost
        try:
            torch.autograd.Variable._execution_engine.queue_callback(slot.flush)
        except RuntimeError:
            return None
        slot.task = task
    return slot


def pending_tails() -> int:
    """How many deferred reductions are waiting to run (0 outside a backward pass)."""
    return sum(1 for s in _tail_slots.values() if s.pending is not None)


# set to a list to receive, per set-abstraction forward call, {"neighbours": (B,S,K) int32 | None, "argmax": (B,S,C) int32}
# (views into the call's saved workspace) -- used by the parity tests to hand the fp64 oracle the same max-pool routing
sa_tap: Optional[list] = None


class _SetAbstraction(torch.autograd.Function):
    """PointNetSetAbstraction.forward / backward as two C calls (models/pointnet_pp_8dir.py:21-43)."""

    @staticmethod
    def forward(ctx, xyz, points, centre_idx, neighbour_idx, cfg, running, *params):
        # params: L x (conv_w, conv_b, bn_w, bn_b); running: L x (running_mean, running_var)
        K, group_all, training, eps, momentum, sinks, nbt, pre = cfg
        Lh = len(params) // 4
        xyz = _f32(xyz, "xyz")
        B, N, _ = xyz.shape
        D = 0
        if points is not None:
            points = _f32(points, "points")
            D = points.shape[2]
        conv_w = [_f32(params[4 * l], "conv weight") for l in range(Lh)]
        conv_b = [_f32(params[4 * l + 1], "conv bias") for l in range(Lh)]
        bn_w = [_f32(params[4 * l + 2], "bn weight") for l in range(Lh)]
        bn_b = [_f32(params[4 * l + 3], "bn bias") for l in range(Lh)]
        channels = [w.shape[0] for w in conv_w]
        if group_all:
            S, Kk = 1, N
        else:
            centre_idx = _i32(centre_idx, "centre_idx")
            S, Kk = centre_idx.shape[1], int(K)
            if neighbour_idx is not None:
                neighbour_idx = _i32(neighbour_idx, "neighbour_idx")
        desc = _sa_desc(B, N, S, Kk, D, channels, group_all, training, eps, momentum)
        lib = L.lib()
        sb = lib.pnpp_sa_saved_bytes(C.byref(desc))
        if sb == 0:
            L.check(L.PNPP_ERR_ARG if L.last_error() else L.PNPP_ERR_ARG)
        if pre is not None:   # grouped ahead of time (group_pair): neighbours and centres already sit in this call's workspace
            saved, new_xyz = pre["saved"], pre["new_xyz"]
            if saved.numel() != sb or tuple(new_xyz.shape) != (B, S, 3) or neighbour_idx is not None:
                raise ValueError("set_abstraction: the pre-grouped workspace does not belong to this call")
        else:
            saved = torch.empty(sb, dtype=torch.uint8, device=xyz.device)
            new_xyz = torch.empty(B, S, 3, device=xyz.device, dtype=torch.float32)
        scratch = _scratch(lib.pnpp_sa_scratch_bytes(C.byref(desc)), xyz.device)
        out = torch.empty(B, S, channels[-1], device=xyz.device, dtype=torch.float32)
        a = L.SaFwdArgs()
        a.xyz, a.points = xyz.data_ptr(), _p(points)
        a.centre_idx = None if group_all else centre_idx.data_ptr()
        a.neighbour_idx = _p(neighbour_idx)
        if pre is not None:   # "already in place": the neighbour argument IS the workspace's own index block
            a.neighbour_idx = lib.pnpp_sa_saved_neighbours(C.byref(desc), saved.data_ptr())
        a.conv_w, a.conv_b, a.bn_w, a.bn_b = _ptr_array(conv_w), _ptr_array(conv_b), _ptr_array(bn_w), _ptr_array(bn_b)
        a.bn_rm = _ptr_array([running[2 * l] for l in range(Lh)])
        a.bn_rv = _ptr_array([running[2 * l + 1] for l in range(Lh)])
        a.bn_nbt = _ptr_array(nbt if nbt is not None else [None] * Lh)
        a.new_xyz, a.out, a.saved, a.scratch = new_xyz.data_ptr(), out.data_ptr(), saved.data_ptr(), scratch.data_ptr()
        L.check(lib.pnpp_sa_forward(C.byref(desc), C.byref(a), _stream()))
        ctx.desc = desc
        ctx.sinks = sinks
        ctx.w0 = params[0]   # backward asks it whether its sink has had a second user since (grad_sink)
        ctx.has_points = points is not None
        # which kernels a level takes depends on process-wide switches (bf16 operands, SyncBN); a level on raw coordinates keeps no
        # Z_0 for the generic backward kernels, so its backward pass must run under the switches its forward pass ran under
        ctx.path_state = (lib.pnpp_get_matmul_precision(), lib.pnpp_stats_exchange_enabled(), lib.pnpp_get_split_products())
        ctx.save_for_backward(xyz, points if points is not None else xyz.new_empty(0), saved, *conv_w, *bn_w, *bn_b)
        if group_all:
            nbr = torch.empty(0, dtype=torch.int32, device=xyz.device)
        else:  # view of the neighbour indices kept in the saved workspace
            off = lib.pnpp_sa_saved_neighbours(C.byref(desc), saved.data_ptr()) - saved.data_ptr()
            nbr = saved[off:off + 4 * B * S * Kk].view(torch.int32).view(B, S, Kk)
        if sa_tap is not None:   # diagnostics: views of what backward will route by (neighbour rows, max-pool positions)
            aoff = lib.pnpp_sa_saved_argmax(C.byref(desc), saved.data_ptr()) - saved.data_ptr()
            arg = saved[aoff:aoff + 4 * B * S * channels[-1]].view(torch.int32).view(B, S, channels[-1])
            # ... and of every ReLU decision the backward pass will take (pnpp_sa_saved_relu_mask), per layer (B, S, K, C_l) uint8
            masks = []
            for l in range(Lh):
                m = torch.empty(B, S, Kk, channels[l], device=xyz.device, dtype=torch.uint8)
                L.check(lib.pnpp_sa_saved_relu_mask(C.byref(desc), saved.data_ptr(), xyz.data_ptr(), conv_w[0].data_ptr(), l,
                                                    m.data_ptr(), _stream()))
                masks.append(m)
            sa_tap.append({"neighbours": None if group_all else nbr, "argmax": arg, "relu_masks": masks})
        ctx.mark_non_differentiable(new_xyz, nbr)
        ctx.set_materialize_grads(False)  # no zero tensors (= fill launches) for the two outputs that carry no gradient
        return new_xyz, out, nbr

    @staticmethod
    def backward(ctx, _dnew_xyz, dout, _dnbr):
        desc = ctx.desc
        Lh = desc.L
        if dout is None:
            return (None,) * (6 + 4 * Lh)
        t = ctx.saved_tensors
        xyz, points, saved = t[0], (t[1] if ctx.has_points else None), t[2]
        conv_w, bn_w, bn_b = t[3:3 + Lh], t[3 + Lh:3 + 2 * Lh], t[3 + 2 * Lh:3 + 3 * Lh]
        dout = _f32(dout, "dout")
        lib = L.lib()
        if ctx.path_state != (lib.pnpp_get_matmul_precision(), lib.pnpp_stats_exchange_enabled(), lib.pnpp_get_split_products()):
            raise ValueError("set_abstraction: matmul precision or SyncBN was switched between this level's forward pass and its "
                             "backward pass; the kept workspace belongs to the kernels the forward pass took")
        # gradient destinations, kind by kind (a conv bias is not kept for the backward pass: it has its BatchNorm weight's shape)
        sinks = ctx.sinks or [None] * (4 * Lh)
        d_conv_w, r_conv_w = _grad_dests(conv_w, sinks[0::4])
        d_conv_b, r_conv_b = _grad_dests(bn_w, sinks[1::4])
        d_bn_w, r_bn_w = _grad_dests(bn_w, sinks[2::4])
        d_bn_b, r_bn_b = _grad_dests(bn_b, sinks[3::4])
        dpoints = torch.empty_like(points) if (points is not None and ctx.needs_input_grad[1]) else None
        a = L.SaBwdArgs()
        a.xyz, a.points = xyz.data_ptr(), _p(points)
        a.conv_w, a.bn_w, a.bn_b = _ptr_array(conv_w), _ptr_array(bn_w), _ptr_array(bn_b)
        a.dout, a.saved = dout.data_ptr(), saved.data_ptr()
        a.d_conv_w, a.d_conv_b = _ptr_array(d_conv_w), _ptr_array(d_conv_b)
        a.d_bn_w, a.d_bn_b = _ptr_array(d_bn_w), _ptr_array(d_bn_b)
        a.dpoints = _p(dpoints)
        # The level's last reduction (dW_0) may wait for the next level's pooling launch only where nothing reads it before the pass
        # ends: its destination is an optimiser's buffer.  A gradient returned to autograd is accumulated as soon as this returns.
        # Nor where a second use of the weight adds to that buffer during the pass (grad_sink marks the sink shared).
        slot = _tail_slot(xyz.device) if (r_conv_w[0] is None and not getattr(ctx.w0, "_pnpp_sink_shared", False)) else None
        if slot is None:
            a.scratch = _scratch(lib.pnpp_sa_scratch_bytes(C.byref(desc)), xyz.device).data_ptr()   # runs what the level before left
            L.check(lib.pnpp_sa_backward(C.byref(desc), C.byref(a), _stream()))
        else:
            scratch = _scratch(lib.pnpp_sa_scratch_bytes(C.byref(desc)), xyz.device, keep_tail=True)
            a.scratch = scratch.data_ptr()
            ride, defer = slot.take(), L.SaTail()
            L.check(lib.pnpp_sa_backward_ex(C.byref(desc), C.byref(a), C.byref(ride[0]) if ride is not None else None, C.byref(defer),
                                            _stream()))
            if defer.kind != L.SA_TAIL_NONE:
                slot.pending = (defer, _stream(), torch.cuda.current_stream(xyz.device), (scratch, d_conv_w[0]))
        grads = [g for layer in zip(r_conv_w, r_conv_b, r_bn_w, r_bn_b) for g in layer]
        return (None, dpoints, None, None, None, None, *grads)


def group_pair(xyz, centre1, centre2, nsample1, convs1, nsample2, convs2, training=True, lengths=None):
    """Centre gather + neighbour search of two stacked set-abstraction levels (sa1 on the cloud, sa2 on sa1's centres) in ONE
    launch, ahead of both forward passes (models/pointnet_pp_8dir.py:28-31 of each level): level 2 searches among level 1's
    centres, which are rows of the same cloud, so it does not wait for level 1's MLP.  centre1 (B,S1) rows of xyz, centre2
    (B,S2) positions among level 1's centres.  Returns the two `pre=` workspaces for set_abstraction; the neighbour sets are
    those the per-level search finds (same coordinates, same arithmetic).  lengths (B,): a ragged batch -- level 1 searches
    xyz[b, :lengths[b]] (same launch, same grid; level 2 searches level 1's centres and is uniform either way)."""
    xyz = _f32(xyz, "xyz")
    B, N, _ = xyz.shape
    c1, c2 = _i32(centre1, "centre_idx"), _i32(centre2, "centre_idx")
    S1, S2 = c1.shape[1], c2.shape[1]
    ch1, ch2 = [c.weight.shape[0] for c in convs1], [c.weight.shape[0] for c in convs2]
    d1 = _sa_desc(B, N, S1, int(nsample1), 0, ch1, False, training, 1e-5, 0.1)
    d2 = _sa_desc(B, S1, S2, int(nsample2), ch1[-1], ch2, False, training, 1e-5, 0.1)
    lib = L.lib()
    pres = []
    for d, S in ((d1, S1), (d2, S2)):
        pres.append({"saved": _workspace(lib.pnpp_sa_saved_bytes(C.byref(d)), xyz.device),
                     "new_xyz": torch.empty(B, S, 3, device=xyz.device, dtype=torch.float32)})
    tail = (c1.data_ptr(), c2.data_ptr(), pres[0]["saved"].data_ptr(), pres[0]["new_xyz"].data_ptr(), pres[1]["saved"].data_ptr(),
            pres[1]["new_xyz"].data_ptr(), _stream())
    if lengths is not None:
        lengths = ragged_lengths(lengths, B, N, xyz.device, minimum=max(S1, int(nsample1)))
        L.check(lib.pnpp_sa_group_pair_ragged(C.byref(d1), C.byref(d2), xyz.data_ptr(), lengths.data_ptr(), *tail))
    else:
        L.check(lib.pnpp_sa_group_pair(C.byref(d1), C.byref(d2), xyz.data_ptr(), *tail))
    return pres[0], pres[1]


def set_abstraction(xyz, points, centre_idx, nsample, group_all, training, convs, bns, neighbour_idx=None,
                    return_neighbours=False, pre=None):
    """Functional form used by models.pointnet_pp_8dir.PointNetSetAbstraction.

    convs / bns are the nn.Conv2d / nn.BatchNorm2d containers (their tensors are used in place:
    weights are read, running statistics are updated by the kernels when training).
    Returns (new_xyz, new_points) exactly like the reference module.
    """
    params, running = [], []
    for conv, bn in zip(convs, bns):
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
        running += [bn.running_mean, bn.running_var]
    sinks = [grad_sink(p) for p in params]
    nbt = [_nbt(bn) for bn in bns] if training else None   # bumped by the statistics kernels themselves
    cfg = (nsample, bool(group_all), bool(training), bns[0].eps, _bn_momentum(bns[0]), sinks if any(s is not None for s in sinks) else None, nbt, pre)
    new_xyz, out, nbr = _SetAbstraction.apply(xyz, points, centre_idx, neighbour_idx, cfg, running, *params)
    if return_neighbours:
        return new_xyz, out, (None if group_all else nbr)
    return new_xyz, out


# ------------------------------------------------------------------------------------------------
# fully connected block
# ------------------------------------------------------------------------------------------------
def _fc_desc(M, K, N, norm, relu, training, eps, momentum, drop_scale):
    d = L.FcDesc()
    d.M, d.K, d.N, d.norm, d.relu, d.training = int(M), int(K), int(N), norm, int(relu), int(training)
    d.eps, d.momentum, d.drop_scale = float(eps), float(momentum), float(drop_scale)
    return d


def _fc_forward_call(d, x, w, b, nw, nb, rm, rv, nbt, mask, draw):
    """pnpp_fc_forward on checked tensors -> (y, the kept workspace, the keep-mask the backward pass needs).  draw = (p, seed,
    counter): the kernel draws the keep-mask itself (no RNG launch, graph-replayable) and hands it back."""
    lib = L.lib()
    saved = _workspace(lib.pnpp_fc_saved_bytes(C.byref(d)), x.device)
    scratch = _scratch(lib.pnpp_fc_scratch_bytes(C.byref(d)), x.device)
    y = torch.empty(d.M, d.N, device=x.device, dtype=torch.float32)
    if mask is not None:
        mask = mask.contiguous()
    a = L.FcFwdArgs()
    a.x, a.w, a.b, a.nw, a.nb = x.data_ptr(), w.data_ptr(), b.data_ptr(), _p(nw), _p(nb)
    a.rm, a.rv, a.nbt, a.mask = _p(rm), _p(rv), _p(nbt), _p(mask)
    if draw is not None:
        p_drop, seed, counter = draw
        mask = torch.empty(d.M, d.N, device=x.device, dtype=torch.uint8)
        a.mask_out, a.drop_p, a.rng_seed, a.rng_counter = mask.data_ptr(), float(p_drop), int(seed) & (2**64 - 1), counter.data_ptr()
    a.y, a.saved, a.scratch = y.data_ptr(), saved.data_ptr(), scratch.data_ptr()
    L.check(lib.pnpp_fc_forward(C.byref(d), C.byref(a), _stream()))
    return y, saved, mask


def _fc_backward_call(d, x, w, b, nw, nb, mask, dy, saved, want_dx, sinks):
    """pnpp_fc_backward -> (dx or None, the gradients of (w, b, nw, nb) for autograd: None where a sink of `sinks` took one)"""
    lib = L.lib()
    scratch = _scratch(lib.pnpp_fc_scratch_bytes(C.byref(d)), x.device)
    dx = torch.empty_like(x) if want_dx else None
    (dw, db, dnw, dnb), returned = _grad_dests((w, b, nw, nb), sinks)
    a = L.FcBwdArgs()
    a.x, a.w, a.b, a.nw, a.nb, a.mask = x.data_ptr(), w.data_ptr(), b.data_ptr(), _p(nw), _p(nb), _p(mask)
    a.dy, a.saved, a.scratch = dy.data_ptr(), saved.data_ptr(), scratch.data_ptr()
    a.dx, a.dw, a.db, a.dnw, a.dnb = _p(dx), dw.data_ptr(), db.data_ptr(), _p(dnw), _p(dnb)
    L.check(lib.pnpp_fc_backward(C.byref(d), C.byref(a), _stream()))
    return dx, returned


class _FcBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, nw, nb, rm, rv, mask, cfg):
        norm, relu, training, eps, momentum, drop_scale, sinks, nbt, draw = cfg
        x, w, b = _f32(x, "x"), _f32(w, "weight"), _f32(b, "bias")
        if nw is not None:
            nw, nb = _f32(nw, "norm weight"), _f32(nb, "norm bias")
        M, K = x.shape
        d = _fc_desc(M, K, w.shape[0], norm, relu, training, eps, momentum, drop_scale)
        y, saved, mask = _fc_forward_call(d, x, w, b, nw, nb, rm, rv, nbt, mask, draw)
        ctx.desc = d
        ctx.sinks = sinks
        ctx.has_norm, ctx.has_mask = nw is not None, mask is not None
        e = x.new_empty(0)
        ctx.save_for_backward(x, w, b, nw if nw is not None else e, nb if nb is not None else e,
                              mask if mask is not None else e, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, nw, nb, mask, saved = ctx.saved_tensors
        nw, nb = (nw, nb) if ctx.has_norm else (None, None)
        mask = mask if ctx.has_mask else None
        dx, grads = _fc_backward_call(ctx.desc, x, w, b, nw, nb, mask, _f32(dy, "dy"), saved, ctx.needs_input_grad[0], ctx.sinks)
        return (dx, *grads, None, None, None, None)


def fc_block(x, linear, norm=None, relu=False, dropout=None, training=True, mask=None):
    """Linear -> optional BatchNorm1d/LayerNorm -> optional ReLU -> optional dropout.

    `dropout` is an nn.Dropout (its p is used, a fresh keep-mask is drawn on the device in training) or
    None; `mask` injects an explicit (M,N) keep-mask instead (tests / parity runs).
    """
    import torch.nn as nn
    nw = nb = rm = rv = None
    kind, eps, momentum = L.NORM_NONE, 1e-5, 0.1
    if isinstance(norm, nn.BatchNorm1d):
        kind, eps, momentum = L.NORM_BATCH, norm.eps, _bn_momentum(norm)
        nw, nb, rm, rv = norm.weight, norm.bias, norm.running_mean, norm.running_var
    elif isinstance(norm, nn.LayerNorm):
        kind, eps = L.NORM_LAYER, norm.eps
        nw, nb = norm.weight, norm.bias
    elif norm is not None:
        raise TypeError(f"unsupported norm module {type(norm).__name__}")
    drop_scale = 1.0
    draw = None
    if training and mask is None and dropout is not None and dropout.p > 0:
        from . import dist as _pdist
        if x.is_cuda and ((kind == L.NORM_BATCH and x.shape[0] <= 32 and not _pdist.sync_batchnorm_enabled()) or
                          (kind == L.NORM_LAYER and dropout.p < 1.0)):
            # the BatchNorm epilogue / the LayerNorm pass draws it in the kernel (SyncBN takes the unfused route: the mask comes from torch)
            draw = (dropout.p, torch.initial_seed(), _dropout_counter(x.device))
            drop_scale = 1.0 / (1.0 - dropout.p)
        else:
            mask = torch.empty(x.shape[0], linear.weight.shape[0], device=x.device, dtype=torch.uint8).bernoulli_(1.0 - dropout.p)
    if mask is not None:
        if not training:
            mask = None
        else:
            p = dropout.p if dropout is not None else 0.5
            drop_scale = 1.0 / (1.0 - p)
            mask = mask.to(device=x.device, dtype=torch.uint8)
    sinks = tuple(grad_sink(p) for p in (linear.weight, linear.bias, nw, nb))
    nbt = _nbt(norm) if (training and kind == L.NORM_BATCH) else None   # bumped by the statistics kernel itself
    cfg = (kind, relu, training, eps, momentum, drop_scale, sinks if any(s is not None for s in sinks) else None, nbt, draw)
    return _FcBlock.apply(x, linear.weight, linear.bias, nw, nb, rm, rv, mask, cfg)


# ------------------------------------------------------------------------------------------------
# heads and losses
# ------------------------------------------------------------------------------------------------
def _vm_head_kl_call(who, o, mu_gt=None, kappa_gt=None, mean=False):
    """The single-peak head of the raw fc3 output `o` (B,2) and, where targets are given, its KL against them, in one launch:
    pnpp_vm_head_kl (mu, kappa, the loss per sample, d loss / d o) or, mean=True, pnpp_vm_head_kl_mean (the batch mean, d mean / d o).
    Returns (o as float32, mu, kappa, loss, d_o) with None for what the launch does not produce."""
    o = _f32(o, "o")
    gt = mu_gt is not None
    mu_gt, kappa_gt = (_f32(mu_gt, "mu_gt"), _f32(kappa_gt, "kappa_gt")) if gt else (None, None)
    B = o.shape[0]
    if o.dim() != 2 or o.shape[1] != 2 or (gt and (mu_gt.numel() != B or kappa_gt.numel() != B)):
        raise ValueError(f"{who}: o must be (B,2) and the targets (B,), got {[tuple(t.shape) for t in (o, mu_gt, kappa_gt) if t is not None]}")
    new = lambda *shape: torch.empty(shape, device=o.device, dtype=torch.float32)
    mu, kappa = (None, None) if mean else (new(B), new(B))
    loss = new() if mean else new(B) if gt else None
    d_o = torch.empty_like(o) if gt else None
    if mean:
        L.check(L.lib().pnpp_vm_head_kl_mean(o.data_ptr(), mu_gt.data_ptr(), kappa_gt.data_ptr(), B, None, None, None, loss.data_ptr(),
                                             d_o.data_ptr(), _stream()))
    else:
        L.check(L.lib().pnpp_vm_head_kl(o.data_ptr(), _p(mu_gt), _p(kappa_gt), B, mu.data_ptr(), kappa.data_ptr(), _p(loss), _p(d_o),
                                        _stream()))
    return o, mu, kappa, loss, d_o


class _VmHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o):
        o, mu, kappa, _, _ = _vm_head_kl_call("vm_head", o)
        ctx.save_for_backward(o)
        return mu, kappa

    @staticmethod
    def backward(ctx, dmu, dkappa):
        (o,) = ctx.saved_tensors
        B = o.shape[0]
        dmu = _f32(dmu, "dmu") if dmu is not None else torch.zeros(B, device=o.device)
        dkappa = _f32(dkappa, "dkappa") if dkappa is not None else torch.zeros(B, device=o.device)
        d_o = torch.empty_like(o)
        L.check(L.lib().pnpp_vm_head_bwd(o.data_ptr(), dmu.data_ptr(), dkappa.data_ptr(), B, d_o.data_ptr(), _stream()))
        return d_o


def vm_head(o: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """mu = tanh(o[:,0])*pi, kappa = softplus(o[:,1])  (pointnet_pp_vonMises.py:36-37)."""
    return _VmHead.apply(o)


class _KlSingle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu_p, kappa_p, mu_q, kappa_q):
        mu_p, kappa_p = _f32(mu_p, "mu_p"), _f32(kappa_p, "kappa_p")
        mu_q, kappa_q = _f32(mu_q, "mu_q"), _f32(kappa_q, "kappa_q")
        n = mu_p.numel()
        kl, dmu, dk = torch.empty_like(mu_p), torch.empty_like(mu_p), torch.empty_like(mu_p)
        L.check(L.lib().pnpp_vm_kl_single(mu_p.data_ptr(), kappa_p.data_ptr(), mu_q.data_ptr(), kappa_q.data_ptr(), n,
                                          kl.data_ptr(), dmu.data_ptr(), dk.data_ptr(), _stream()))
        ctx.save_for_backward(dmu, dk)
        return kl

    @staticmethod
    def backward(ctx, g):
        dmu, dk = ctx.saved_tensors
        return g * dmu, g * dk, None, None


def kl_von_mises_single(mu_p, kappa_p, mu_q, kappa_q):
    """train_single_peak_vonMises_KL.py:23-28 (value and analytic gradient from one launch)."""
    return _KlSingle.apply(mu_p, kappa_p, mu_q, kappa_q)


def vm_head_kl_fused(o, mu_gt, kappa_gt):
    """fc3 output -> (mu, kappa, loss_vec, d loss_vec/d o) in ONE launch (no autograd graph)."""
    return _vm_head_kl_call("vm_head_kl_fused", o, mu_gt, kappa_gt)[1:]


class _VmHeadKlLoss(torch.autograd.Function):
    """Raw fc3 output -> KL loss (per sample or batch mean) with the head, the loss and their gradient in one launch."""

    @staticmethod
    def forward(ctx, o, mu_gt, kappa_gt, mean):
        ctx.mean = bool(mean)
        *_, loss, d_o = _vm_head_kl_call("vm_head_kl_loss", o, mu_gt, kappa_gt, mean=ctx.mean)
        ctx.save_for_backward(d_o)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_o,) = ctx.saved_tensors
        return (g * d_o if ctx.mean else g[:, None] * d_o), None, None, None


def vm_head_kl_loss(o, mu_gt, kappa_gt, reduction: str = "mean"):
    """KL(vM(head(o)) || vM(mu_gt, kappa_gt)) from the raw fc3 output `o` (B,2): pointnet_pp_vonMises.py:36-37 +
    train_single_peak_vonMises_KL.py:23-28 (+ the `.mean()` of line 83 for reduction="mean") in one launch."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
    return _VmHeadKlLoss.apply(o, mu_gt, kappa_gt, reduction == "mean")


def vm_head_kl_loss_backward(o, mu_gt, kappa_gt) -> torch.Tensor:
    """The training step's `loss = kl(...).mean(); loss.backward()` in one go: the fused launch already produces
    d loss / d o, so the backward pass is seeded with it directly (autograd would otherwise launch a fill for the
    scalar's unit gradient and a multiply by it).  Returns the detached mean loss; gradients of everything upstream of
    `o` are accumulated exactly as by loss.backward()."""
    *_, loss, d_o = _vm_head_kl_call("vm_head_kl_loss_backward", o, mu_gt, kappa_gt, mean=True)
    if o.requires_grad:
        torch.autograd.backward([o], [d_o])
    return loss


def _draw_centres(job) -> None:
    """The centre draw of sampling.CentreRing.job() as a launch of its own: the same draws from the same counter as when it rides in
    a tail launch (a tail that does not take the one-launch form, or a cloud whose candidate table exceeds that launch's LDS)."""
    L.check(L.lib().pnpp_sample_random_dev2(*job.c_args(), _stream()))


def _rider_fits(job, lds_limit: int) -> bool:
    """The riding draw keeps an (N + 1)-entry table of 8-byte candidates in the tail launch's LDS."""
    return 8 * (max(job.N1, job.N2) + 1) <= lds_limit


_NO_RIDER = (0, None, 0, 0, 0, 0, None, 0, 0, None)


def _place_rider(next_centres, lds_limit: Optional[int]):
    """The sampler arguments of a tail's C entry.  The draw `next_centres` (sampling.CentreRing.job(), or None) rides in the tail's launch if
    its table fits `lds_limit` bytes of LDS; else (or lds_limit None: a tail in separate launches) it is launched here: _NO_RIDER, as for None."""
    if next_centres is not None and lds_limit is not None and _rider_fits(next_centres, lds_limit):
        return next_centres.c_args()
    if next_centres is not None:
        _draw_centres(next_centres)
    return _NO_RIDER


def _finish_tail(x, dx, params, fresh) -> None:
    """What is left of `loss.backward()` after a tail's launch: a gradient that no sink took (fresh: _grad_dests' second result) is
    accumulated into its parameter's .grad with plain autograd semantics, and dx seeds the backward pass of everything before x."""
    for p, g in zip(params, fresh):
        if g is not None and p.requires_grad:
            if p.grad is None:
                p.grad = g.view_as(p)
            else:
                p.grad.add_(g.view_as(p))                        # in place: .grad may be a view of a flat buffer
    if dx is not None:
        torch.autograd.backward([x], [dx])


def vm_fc_head_kl_loss_backward(x, linear, mu_gt, kappa_gt, next_centres=None) -> torch.Tensor:
    """`o = linear(x)` (the model's fc3, two outputs), head, single-peak KL, `.mean()` and `loss.backward()` in ONE launch
    (pointnet_pp_vonMises.py:35-37 + train_single_peak_vonMises_KL.py:82-84): the gradients of `linear` land in its
    .grad (or the optimiser's flat buffer), the gradient of x seeds the rest of the backward pass.  Returns the
    detached mean loss.  Equals vm_head_kl_loss_backward(fc_block(x, linear), ...) to float32 rounding."""
    x32, mu_gt, kappa_gt = _f32(x, "x"), _f32(mu_gt, "mu_gt"), _f32(kappa_gt, "kappa_gt")
    w, b = _f32(linear.weight, "weight"), _f32(linear.bias, "bias")
    B, K = x32.shape
    if w.shape != (2, K) or b.numel() != 2 or mu_gt.numel() != B or kappa_gt.numel() != B:
        raise ValueError("vm_fc_head_kl_loss_backward: linear must map K -> 2 and the targets must be (B,)")
    if 4 * (2 * B + 2 * K + 8 + (B * K if B * K <= 12288 else 0)) > 56 * 1024:
        # the one-launch form stages fc3's weights and the outputs in LDS (56 KB); wider heads take the three launches it fuses
        _place_rider(next_centres, None)
        return vm_head_kl_loss_backward(fc_block(x, linear, training=True), mu_gt, kappa_gt)
    rider = _place_rider(next_centres, 56 * 1024)   # clouds of N >= 7168: the draw takes its own launch
    loss = torch.empty((), device=x32.device, dtype=torch.float32)
    params = (linear.weight, linear.bias)
    (dw, db), fresh = _grad_dests((w, b), [grad_sink(p) for p in params])
    dx = torch.empty_like(x32) if x.requires_grad else None
    tail = (x32.data_ptr(), w.data_ptr(), b.data_ptr(), mu_gt.data_ptr(), kappa_gt.data_ptr(), B, K, loss.data_ptr(), dw.data_ptr(),
            db.data_ptr(), _p(dx))
    if rider is _NO_RIDER:
        L.check(L.lib().pnpp_vm_fc_head_kl_step(*tail, _stream()))
    else:
        L.check(L.lib().pnpp_vm_fc_head_kl_step_sample(*tail, *rider, _stream()))
    _finish_tail(x, dx, params, fresh)
    return loss


def mvm_heads_match_loss_backward(x, head_pi, head_mu, head_kappa, vm_gt, K_gt, temp, kappa_max, next_centres=None, outputs=False):
    """The three output heads of PointNetPPMvM on features `x` (B,K), the head activations, `match_loss(...).mean()` and
    `loss.backward()` in ONE launch (models/pointnet_pp_mvM.py:91-125 + train_multi_peaks_vonMises_KL.py:54-81, :229-234): the
    heads' gradients land in their .grad (or the optimiser's flat buffer), the gradient of x seeds the rest of the backward pass.
    Returns the detached mean loss (and mu, kappa, weight with outputs=True).  Equals
    match_loss(*mvm_head(fc_block(x, head_pi), fc_block(x, head_mu), fc_block(x, head_kappa), ...), vm_gt, K_gt).mean() + backward()
    to float32 rounding; max_K other than 4 / 8 or heads too wide for the launch's LDS take exactly that route."""
    x32, vm_gt = _f32(x, "x"), _f32(vm_gt, "vm_gt")
    K32 = _i32(K_gt, "K_gt")
    B, K = x32.shape
    maxK = head_pi.weight.shape[0]
    heads = (head_pi, head_mu, head_kappa)
    # the one-launch form stages x with 16-byte loads: K % 4 == 0 and an aligned x (a contiguous view may start anywhere)
    fits = (maxK in (4, 8) and K % 4 == 0 and x32.data_ptr() % 16 == 0
            and 4 * (4 * maxK * (B + K) + B * K + 3 * B * maxK * (1 + maxK)) <= 96 * 1024)
    if (head_mu.weight.shape[0] != 2 * maxK or head_kappa.weight.shape[0] != maxK or any(h.weight.shape[1] != K for h in heads)
            or tuple(vm_gt.shape) != (B, maxK, 3)):
        raise ValueError("mvm_heads_match_loss_backward: heads must map K -> max_K / 2 max_K / max_K and vm_gt must be (B, max_K, 3)")
    if not fits:
        _place_rider(next_centres, None)
        mu, kappa, weight = mvm_head(*[fc_block(x, h, training=True) for h in heads], temp, kappa_max)
        loss = match_loss(mu, kappa, weight, vm_gt, K_gt).mean()
        loss.backward()
        loss = loss.detach()
        return (loss, mu.detach(), kappa.detach(), weight.detach()) if outputs else loss
    rider = _place_rider(next_centres, 96 * 1024)   # clouds of N >= 12288: the draw takes its own launch
    params = [p for h in heads for p in (h.weight, h.bias)]
    wb = [_f32(t, name) for h in heads for t, name in ((h.weight, "weight"), (h.bias, "bias"))]
    loss = torch.empty((), device=x32.device, dtype=torch.float32)
    grads, fresh = _grad_dests(wb, [grad_sink(p) for p in params])
    dx = torch.empty_like(x32) if x.requires_grad else None
    outs = [torch.empty(B, maxK, device=x32.device, dtype=torch.float32) for _ in range(3)] if outputs else [None] * 3
    L.check(L.lib().pnpp_mvm_fc_head_match_step(x32.data_ptr(), *[t.data_ptr() for t in wb], vm_gt.data_ptr(), K32.data_ptr(), B, K, maxK,
                                                float(temp), float(kappa_max), loss.data_ptr(), *[g.data_ptr() for g in grads], _p(dx),
                                                *[_p(t) for t in outs], *rider, _stream()))
    _finish_tail(x, dx, params, fresh)
    return (loss, *outs) if outputs else loss


class _MatchLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, kappa, w, vm_gt, K_gt):
        mu, kappa, w, vm_gt = _f32(mu, "mu"), _f32(kappa, "kappa"), _f32(w, "w"), _f32(vm_gt, "vm_gt")
        K32 = _i32(K_gt, "K_gt")
        B, maxK = mu.shape
        lv = torch.empty(B, device=mu.device, dtype=torch.float32)
        dmu, dk, dw = torch.empty_like(mu), torch.empty_like(mu), torch.empty_like(mu)
        assign = torch.empty(B, maxK, device=mu.device, dtype=torch.int32)
        L.check(L.lib().pnpp_vm_match_loss(mu.data_ptr(), kappa.data_ptr(), w.data_ptr(), vm_gt.data_ptr(), K32.data_ptr(), B,
                                           maxK, lv.data_ptr(), dmu.data_ptr(), dk.data_ptr(), dw.data_ptr(),
                                           assign.data_ptr(), _stream()))
        ctx.save_for_backward(dmu, dk, dw)
        ctx.assign = assign
        return lv

    @staticmethod
    def backward(ctx, g):
        dmu, dk, dw = ctx.saved_tensors
        g = g[:, None]
        return g * dmu, g * dk, g * dw, None, None


def match_loss(mu, kappa, w, vm_gt, K_gt):
    """train_multi_peaks_vonMises_KL.py:54-81, whole batch in one launch, no host round trip."""
    return _MatchLoss.apply(mu, kappa, w, vm_gt, K_gt)


class _MvmHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pi_raw, mu_raw, kappa_raw, temp, kappa_max):
        pi_raw, mu_raw, kappa_raw = _f32(pi_raw, "pi_raw"), _f32(mu_raw, "mu_raw"), _f32(kappa_raw, "kappa_raw")
        B, K = pi_raw.shape
        mu, kappa, weight = torch.empty_like(pi_raw), torch.empty_like(pi_raw), torch.empty_like(pi_raw)
        L.check(L.lib().pnpp_mvm_head(pi_raw.data_ptr(), mu_raw.data_ptr(), kappa_raw.data_ptr(), B, K, float(temp),
                                      float(kappa_max), mu.data_ptr(), kappa.data_ptr(), weight.data_ptr(), _stream()))
        ctx.save_for_backward(pi_raw, mu_raw, kappa_raw, weight)
        ctx.cfg = (float(temp), float(kappa_max))
        return mu, kappa, weight

    @staticmethod
    def backward(ctx, dmu, dkappa, dweight):
        pi_raw, mu_raw, kappa_raw, weight = ctx.saved_tensors
        B, K = pi_raw.shape
        z = lambda t: _f32(t, "grad") if t is not None else torch.zeros_like(pi_raw)
        dmu, dkappa, dweight = z(dmu), z(dkappa), z(dweight)
        dpi, dmr, dkr = torch.empty_like(pi_raw), torch.empty_like(mu_raw), torch.empty_like(kappa_raw)
        L.check(L.lib().pnpp_mvm_head_bwd(pi_raw.data_ptr(), mu_raw.data_ptr(), kappa_raw.data_ptr(), weight.data_ptr(),
                                          dmu.data_ptr(), dkappa.data_ptr(), dweight.data_ptr(), B, K, ctx.cfg[0], ctx.cfg[1],
                                          dpi.data_ptr(), dmr.data_ptr(), dkr.data_ptr(), _stream()))
        return dpi, dmr, dkr, None, None


def mvm_head(pi_raw, mu_raw, kappa_raw, temp: float, kappa_max: Optional[float]):
    return _MvmHead.apply(pi_raw, mu_raw, kappa_raw, temp, float("inf") if kappa_max is None else kappa_max)


def _rows(t: torch.Tensor, name: str, shape) -> torch.Tensor:
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _grid_kl_args(first: torch.Tensor, name: str, vm_gt, K_gt, num):
    """Shapes of the two mixture-KL ops: `first` (B, max_K) with max_K <= 8, vm_gt (B, max_K, 3), K_gt (B,), 2 <= num - 1 <= 1024."""
    if first.dim() != 2:
        raise ValueError(f"{name} has shape {tuple(first.shape)}, expected (B, max_K)")
    B, maxK = first.shape
    if B < 1 or not 1 <= maxK <= 8:
        raise ValueError(f"{name} has shape {tuple(first.shape)}: 1 <= B and 1 <= max_K <= 8")
    if not 2 <= int(num) - 1 <= 1024:
        raise ValueError(f"num={num}: a grid of num - 1 points, 2 <= num - 1 <= 1024")
    return B, maxK, _rows(_f32(vm_gt, "vm_gt"), "vm_gt", (B, maxK, 3)), _rows(_i32(K_gt, "K_gt"), "K_gt", (B,))


class _MvmGridKl(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, kappa, w, vm_gt, K_gt, num):
        mu = _f32(mu, "mu")
        B, maxK, vm_gt, K32 = _grid_kl_args(mu, "mu", vm_gt, K_gt, num)
        kappa, w = _rows(_f32(kappa, "kappa"), "kappa", (B, maxK)), _rows(_f32(w, "weight"), "weight", (B, maxK))
        lv = torch.empty(B, device=mu.device, dtype=torch.float32)
        grads = [torch.empty_like(mu) for _ in range(3)] if any(ctx.needs_input_grad[:3]) else [None] * 3
        L.check(L.lib().pnpp_mvm_grid_kl(mu.data_ptr(), kappa.data_ptr(), w.data_ptr(), vm_gt.data_ptr(), K32.data_ptr(), B, maxK,
                                         int(num), lv.data_ptr(), _p(grads[0]), _p(grads[1]), _p(grads[2]), _stream()))
        if grads[0] is not None:
            ctx.save_for_backward(*grads)
        return lv

    @staticmethod
    def backward(ctx, g):
        dmu, dk, dw = ctx.saved_tensors
        g = g[:, None]
        return g * dmu, g * dk, g * dw, None, None, None


def mvm_grid_kl(mu, kappa, weight, vm_gt, K_gt, num: int = 360):
    """KL(ground truth || prediction) of two von-Mises mixtures on decode's grid of num - 1 angles, per sample (B,): every predicted
    component counts, with the weight the head gave it (pnpp_mvm_grid_kl).  Value and gradients in one launch, no host round trip."""
    return _MvmGridKl.apply(mu, kappa, weight, vm_gt, K_gt, num)


class _MvmHeadGridKl(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pi_raw, mu_raw, kappa_raw, vm_gt, K_gt, temp, kappa_max, num, outputs):
        pi_raw = _f32(pi_raw, "pi_raw")
        B, maxK, vm_gt, K32 = _grid_kl_args(pi_raw, "pi_raw", vm_gt, K_gt, num)
        mu_raw = _rows(_f32(mu_raw, "mu_raw"), "mu_raw", (B, 2 * maxK))
        kappa_raw = _rows(_f32(kappa_raw, "kappa_raw"), "kappa_raw", (B, maxK))
        lv = torch.empty(B, device=pi_raw.device, dtype=torch.float32)
        grads = [None] * 3
        if any(ctx.needs_input_grad[:3]):
            grads = [torch.empty_like(pi_raw), torch.empty_like(mu_raw), torch.empty_like(kappa_raw)]
        outs = [torch.empty_like(pi_raw) for _ in range(3)] if outputs else [None] * 3
        L.check(L.lib().pnpp_mvm_head_grid_kl(pi_raw.data_ptr(), mu_raw.data_ptr(), kappa_raw.data_ptr(), vm_gt.data_ptr(), K32.data_ptr(),
                                              B, maxK, float(temp), float(kappa_max), int(num), lv.data_ptr(), _p(grads[0]), _p(grads[1]),
                                              _p(grads[2]), _p(outs[0]), _p(outs[1]), _p(outs[2]), _stream()))
        if grads[0] is not None:
            ctx.save_for_backward(*grads)
        if not outputs:
            return lv
        ctx.mark_non_differentiable(*outs)
        return (lv, *outs)

    @staticmethod
    def backward(ctx, g, *_):
        dpi, dmr, dkr = ctx.saved_tensors
        g = g[:, None]
        return g * dpi, g * dmr, g * dkr, None, None, None, None, None, None


def mvm_head_grid_kl(pi_raw, mu_raw, kappa_raw, vm_gt, K_gt, temp: float, kappa_max: Optional[float], num: int = 360,
                     outputs: bool = False):
    """mvm_head followed by mvm_grid_kl, and their backward, in one launch (pnpp_mvm_head_grid_kl): raw head outputs -> loss (B,), and
    with outputs=True also the detached mu, kappa, weight (B, max_K) of the head."""
    return _MvmHeadGridKl.apply(pi_raw, mu_raw, kappa_raw, vm_gt, K_gt, temp, float("inf") if kappa_max is None else kappa_max, num,
                                outputs)


@torch.no_grad()
def mvm_decode(mu, kappa, weight=None, counts=None, num: int = 360, rel_height: float = 0.1, density: bool = False):
    """pnpp_mvm_decode: mixture parameters (B,K) -> (modes (B,K), heights (B,K), n_modes (B,) int32, angle (B,), density (B,num-1) or
    None); one launch, no host round trip.  mu, kappa (B,): the single-peak model, K = 1 and weight 1."""
    mu, kappa = _f32(mu, "mu"), _f32(kappa, "kappa")
    if mu.dim() == 1:
        mu, kappa = mu[:, None], _rows(kappa, "kappa", mu.shape)[:, None]
    if mu.dim() != 2:
        raise ValueError(f"mu has shape {tuple(mu.shape)}, expected (B, K) or (B,)")
    B, K = mu.shape
    _rows(kappa, "kappa", (B, K))
    weight = None if weight is None else _rows(_f32(weight, "weight"), "weight", (B, K))
    counts = None if counts is None else _rows(_i32(counts, "counts"), "counts", (B,))
    dev = mu.device
    modes, heights = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev)
    n_modes, angle = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev)
    dens = torch.empty(B, max(int(num) - 1, 0), device=dev) if density else None
    L.check(L.lib().pnpp_mvm_decode(mu.data_ptr(), kappa.data_ptr(), _p(weight), _p(counts), B, K, int(num), float(rel_height),
                                    modes.data_ptr(), heights.data_ptr(), n_modes.data_ptr(), angle.data_ptr(), _p(dens), _stream()))
    return modes, heights, n_modes, angle, dens


@torch.no_grad()
def orient_eval(modes, n_modes, angle, mu_gt=None, kappa_gt=None, vm_gt=None, K_gt=None, labels=None, n_labels: int = 1, acc=None,
                sample_err=None, per_sample: bool = True):
    """pnpp_orient_eval: angular errors of decoded orientations against (mu_gt, kappa_gt) (B,) or (vm_gt (B,Kmax,3), K_gt (B,)).
    acc: the int64 accumulator of n_labels * ORIENT_STRIDE + 1 words to add to; sample_err (capacity, 2): the per-sample rows.
    per_sample: also return (top1, cover, count_ok) of this batch (else None)."""
    modes = _f32(modes, "modes")
    if modes.dim() != 2:
        raise ValueError(f"modes has shape {tuple(modes.shape)}, expected (B, K)")
    B, K = modes.shape
    n_modes, angle = _rows(_i32(n_modes, "n_modes"), "n_modes", (B,)), _rows(_f32(angle, "angle"), "angle", (B,))
    Kmax = 0
    if vm_gt is not None:
        vm_gt = _f32(vm_gt, "vm_gt")
        if vm_gt.dim() != 3 or vm_gt.size(0) != B or vm_gt.size(2) != 3:
            raise ValueError(f"vm_gt has shape {tuple(vm_gt.shape)}, expected ({B}, Kmax, 3)")
        Kmax = vm_gt.size(1)
    K_gt = None if K_gt is None else _rows(_i32(K_gt, "K_gt"), "K_gt", (B,))
    mu_gt = None if mu_gt is None else _rows(_f32(mu_gt, "mu_gt"), "mu_gt", (B,))
    kappa_gt = None if kappa_gt is None else _rows(_f32(kappa_gt, "kappa_gt"), "kappa_gt", (B,))
    labels = None if labels is None else _rows(_i32(labels, "labels"), "labels", (B,))
    if acc is not None:
        _need_gpu(acc, "acc")
        if acc.dtype != torch.int64 or not acc.is_contiguous() or acc.numel() != int(n_labels) * L.ORIENT_STRIDE + 1:
            raise ValueError(f"acc must be a contiguous int64 tensor of n_labels * {L.ORIENT_STRIDE} + 1 = "
                             f"{int(n_labels) * L.ORIENT_STRIDE + 1} words, got {acc.dtype} x {acc.numel()}")
    cap = 0
    if sample_err is not None:
        _need_gpu(sample_err, "sample_err")
        if sample_err.dtype != torch.float32 or not sample_err.is_contiguous() or sample_err.dim() != 2 or sample_err.size(1) != 2:
            raise ValueError(f"sample_err must be a contiguous float32 tensor of shape (capacity, 2), got {tuple(sample_err.shape)}")
        cap = sample_err.size(0)
    dev = modes.device
    top1 = torch.empty(B, device=dev) if per_sample else None
    cover = torch.empty(B, device=dev) if per_sample else None
    ok = torch.empty(B, device=dev, dtype=torch.int32) if per_sample else None
    L.check(L.lib().pnpp_orient_eval(modes.data_ptr(), n_modes.data_ptr(), angle.data_ptr(), B, K, _p(mu_gt), _p(kappa_gt), _p(vm_gt),
                                     _p(K_gt), Kmax, _p(labels), int(n_labels), _p(acc), _p(sample_err), cap, _p(top1), _p(cover),
                                     _p(ok), _stream()))
    return top1, cover, ok


class _SoftCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, p):
        logits, p = _f32(logits, "logits"), _f32(p, "p_target")
        B, Cc = logits.shape
        lv, dl = torch.empty(B, device=logits.device, dtype=torch.float32), torch.empty_like(logits)
        L.check(L.lib().pnpp_soft_ce(logits.data_ptr(), p.data_ptr(), B, Cc, lv.data_ptr(), dl.data_ptr(), _stream()))
        ctx.save_for_backward(dl)
        return lv

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return g[:, None] * dl, None


def soft_ce(logits, p_target):
    """train_8dir_KL.py:60-68."""
    return _SoftCE.apply(logits, p_target)


class _LogSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32(x, "x")
        if x.dim() != 2:
            raise ValueError(f"log_softmax takes (M, C) rows, got {tuple(x.shape)}")
        M, Cc = x.shape
        y = torch.empty_like(x)
        L.check(L.lib().pnpp_log_softmax(x.data_ptr(), M, Cc, y.data_ptr(), _stream()))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _f32(dy, "dy")
        dx = torch.empty_like(y)
        L.check(L.lib().pnpp_log_softmax_bwd(y.data_ptr(), dy.data_ptr(), y.shape[0], y.shape[1], dx.data_ptr(), _stream()))
        return dx


def log_softmax(x):
    """F.log_softmax(x, dim=1) of (M, C) rows (PointNet++Demo.py:234)."""
    return _LogSoftmax.apply(x)


class _NllLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, target, check):
        logp = _f32(logp, "logp")
        target = _i32(target, "target")
        if logp.dim() != 2 or target.shape != (logp.shape[0],):
            raise ValueError(f"nll_loss takes logp (M, C) and target (M,), got {tuple(logp.shape)} and {tuple(target.shape)}")
        M, Cc = logp.shape
        loss = torch.empty((), device=logp.device, dtype=torch.float32)
        bad = torch.empty(1, device=logp.device, dtype=torch.int32)
        L.check(L.lib().pnpp_nll_loss(logp.data_ptr(), target.data_ptr(), M, Cc, loss.data_ptr(), bad.data_ptr(), int(check), _stream()))
        ctx.save_for_backward(target)
        ctx.C = Cc
        return loss

    @staticmethod
    def backward(ctx, g):
        (target,) = ctx.saved_tensors
        g = _f32(g, "grad")
        M = target.shape[0]
        dlogp = torch.empty(M, ctx.C, device=target.device, dtype=torch.float32)
        L.check(L.lib().pnpp_nll_loss_bwd(target.data_ptr(), g.data_ptr(), M, ctx.C, dlogp.data_ptr(), _stream()))
        return dlogp, None, None


def nll_loss(logp, target, check: bool = True):
    """F.nll_loss(logp, target) with the default mean reduction (PointNet++Demo.py:244); there is no ignore_index.  A target outside
    [0, C) raises RuntimeError (PNPP_ERR_RANGE): the targets live on the device, so the call waits for the stream to read the kernel's
    count.  check=False skips the wait (stream capture); such a target then adds nothing to the sum and gets no gradient."""
    return _NllLoss.apply(logp, target, check)


def linear_log_softmax(x, linear):
    """log_softmax(linear(x), dim=1) as one launch, forward only (the tail of the classifier's Predictor)."""
    x, w, b = _f32(x, "x"), _f32(linear.weight, "weight"), _f32(linear.bias, "bias")
    M, K = x.shape
    y = torch.empty(M, w.shape[0], device=x.device, dtype=torch.float32)
    L.check(L.lib().pnpp_linear_log_softmax(x.data_ptr(), w.data_ptr(), b.data_ptr(), M, K, w.shape[0], y.data_ptr(), _stream()))
    return y


# ------------------------------------------------------------------------------------------------
# direction-vector heads and losses of the other set-abstraction models
# ------------------------------------------------------------------------------------------------
class _L2Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        x = _f32(x, "x")
        if x.dim() != 2:
            raise ValueError(f"l2_normalize: expected (M,C), got {tuple(x.shape)}")
        M, Cc = x.shape
        y = torch.empty_like(x)
        L.check(L.lib().pnpp_l2_normalize(x.data_ptr(), M, Cc, float(eps), y.data_ptr(), _stream()))
        ctx.save_for_backward(x)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _f32(dy, "dy")
        dx = torch.empty_like(x)
        L.check(L.lib().pnpp_l2_normalize_bwd(x.data_ptr(), dy.data_ptr(), x.shape[0], x.shape[1], ctx.eps, dx.data_ptr(),
                                              _stream()))
        return dx, None


def l2_normalize(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """F.normalize(x, p=2, dim=1, eps) for (M,C) inputs (pointnet_pp_Fwd.py:98, Pointnet_pp_xyz.py:84-85)."""
    return _L2Normalize.apply(x, eps)


class _Mse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t):
        p, t = _f32(p, "input"), _f32(t, "target")
        if p.shape != t.shape:
            raise ValueError(f"mse_loss: input {tuple(p.shape)} and target {tuple(t.shape)} differ")
        loss = torch.empty((), device=p.device, dtype=torch.float32)
        dp = torch.empty_like(p)
        L.check(L.lib().pnpp_mse(p.data_ptr(), t.data_ptr(), p.numel(), loss.data_ptr(), dp.data_ptr(), _stream()))
        ctx.save_for_backward(dp)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return g * dp, None


def mse_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """nn.MSELoss()(pred, target): mean over all elements, value and gradient from one launch."""
    return _Mse.apply(pred, target)


class _MseRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t):
        p, t = _f32(p, "input"), _f32(t, "target")
        if p.shape != t.shape or p.dim() != 2:
            raise ValueError(f"mse_rows: expected two (B,C) tensors, got {tuple(p.shape)} and {tuple(t.shape)}")
        lv, dp = torch.empty(p.shape[0], device=p.device, dtype=torch.float32), torch.empty_like(p)
        L.check(L.lib().pnpp_mse_rows(p.data_ptr(), t.data_ptr(), p.shape[0], p.shape[1], lv.data_ptr(), dp.data_ptr(), _stream()))
        ctx.save_for_backward(dp)
        return lv

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return g[:, None] * dp, None


def mse_rows(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Per-sample mean squared error (B,C) -> (B,) (simple_pointnet_train.py:174); its mean is nn.MSELoss()(pred, target)."""
    return _MseRows.apply(pred, target)


class _Orth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32(a, "a"), _f32(b, "b")
        if a.shape != b.shape or a.dim() != 2:
            raise ValueError(f"orth_loss: expected two (B,C) tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
        loss = torch.empty((), device=a.device, dtype=torch.float32)
        da, db = torch.empty_like(a), torch.empty_like(b)
        L.check(L.lib().pnpp_orth_loss(a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], loss.data_ptr(), da.data_ptr(),
                                       db.data_ptr(), _stream()))
        ctx.save_for_backward(da, db)
        return loss

    @staticmethod
    def backward(ctx, g):
        da, db = ctx.saved_tensors
        return g * da, g * db


def orth_loss(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(a * b).sum(1).pow(2).mean()  (train.py:184-185)."""
    return _Orth.apply(a, b)


class _ProjProbs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vec, dirs):
        vec, dirs = _f32(vec, "vec"), _f32(dirs, "dirs")
        if vec.dim() != 2 or vec.shape[1] != 3 or dirs.dim() != 2 or dirs.shape[1] != 3:
            raise ValueError(f"proj_probs: expected vec (B,3) and dirs (D,3), got {tuple(vec.shape)}, {tuple(dirs.shape)}")
        B, D = vec.shape[0], dirs.shape[0]
        probs = torch.empty(B, D, device=vec.device, dtype=torch.float32)
        L.check(L.lib().pnpp_proj_probs(vec.data_ptr(), dirs.data_ptr(), B, D, probs.data_ptr(), _stream()))
        ctx.save_for_backward(vec, dirs)
        return probs

    @staticmethod
    def backward(ctx, dprobs):
        vec, dirs = ctx.saved_tensors
        dprobs = _f32(dprobs, "dprobs")
        dvec = torch.empty_like(vec)
        L.check(L.lib().pnpp_proj_probs_bwd(vec.data_ptr(), dirs.data_ptr(), dprobs.data_ptr(), vec.shape[0], dirs.shape[0],
                                            dvec.data_ptr(), _stream()))
        return dvec, None


def proj_probs(vec: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """train_multi_8dir.py:41-44: unit vector -> non-negative cosine to each of the D directions -> normalised to sum 1."""
    return _ProjProbs.apply(vec, dirs)


# ------------------------------------------------------------------------------------------------
# vanilla PointNet (models/pointnet.py): pooled wide layer, per-cloud transforms, regulariser, head pieces.
# float32 products whatever set_matmul_precision / set_float32_products say (those switch the set-abstraction GEMMs only).
# ------------------------------------------------------------------------------------------------
# set to a list to receive, per pooled-layer forward call, {"route": (B,C) int32, "zsel": (B,C) float32} (views into the call's
# saved workspace): the row each pooled value came from and z there -- the parity tests hand these to a float64 evaluation
pn_pool_tap: Optional[list] = None


def _pn_pool_desc(B, N, K, C_, relu, training, eps, momentum):
    d = L.PnPoolDesc()
    d.B, d.N, d.K, d.C, d.relu, d.training = int(B), int(N), int(K), int(C_), int(relu), int(training)
    d.eps, d.momentum = float(eps), float(momentum)
    return d


def _pn_pool_forward_call(d, a, w, b, gamma, beta, rm, rv, nbt, rag):
    """pnpp_pn_pool_forward(_ragged) on checked tensors -> (out (B, C), the kept workspace); rag: None or the batch's PackedLengths"""
    lib = L.lib()
    if rag is None:
        sb, scb = lib.pnpp_pn_pool_saved_bytes(C.byref(d)), lib.pnpp_pn_pool_scratch_bytes(C.byref(d))
    else:
        sb, scb = lib.pnpp_pn_pool_saved_bytes_ragged(C.byref(d), rag.M_total), lib.pnpp_pn_pool_scratch_bytes_ragged(C.byref(d), rag.M_total)
    saved = _workspace(sb, a.device)
    scratch = _scratch(scb, a.device)
    out = torch.empty(d.B, d.C, device=a.device, dtype=torch.float32)
    x = L.PnPoolFwdArgs()
    x.a, x.w, x.b, x.gamma, x.beta = a.data_ptr(), w.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    x.rm, x.rv, x.nbt = rm.data_ptr(), rv.data_ptr(), _p(nbt)
    x.out, x.saved, x.scratch = out.data_ptr(), saved.data_ptr(), scratch.data_ptr()
    if rag is None:
        L.check(lib.pnpp_pn_pool_forward(C.byref(d), C.byref(x), _stream()))
    else:
        L.check(lib.pnpp_pn_pool_forward_ragged(C.byref(d), C.byref(x), rag.offs_dev.data_ptr(), rag.M_total, _stream()))
    if pn_pool_tap is not None:
        r = lib.pnpp_pn_pool_saved_route(C.byref(d), saved.data_ptr()) - saved.data_ptr()
        z = lib.pnpp_pn_pool_saved_zsel(C.byref(d), saved.data_ptr()) - saved.data_ptr()
        pn_pool_tap.append({"route": saved[r:r + 4 * d.B * d.C].view(torch.int32).view(d.B, d.C),
                            "zsel": saved[z:z + 4 * d.B * d.C].view(torch.float32).view(d.B, d.C)})
    return out, saved


def _pn_pool_backward_call(d, a, w, gamma, dout, saved, rag, want_da, sinks):
    """pnpp_pn_pool_backward(_ragged) -> (da or None, the gradients of (w, b, gamma, beta) for autograd: None where a sink took one)"""
    lib = L.lib()
    scb = lib.pnpp_pn_pool_scratch_bytes(C.byref(d)) if rag is None else lib.pnpp_pn_pool_scratch_bytes_ragged(C.byref(d), rag.M_total)
    scratch = _scratch(scb, a.device)
    da = torch.empty_like(a) if want_da else None
    (dw, db, dgamma, dbeta), returned = _grad_dests((w, gamma, gamma, gamma), sinks)   # the conv bias and beta have gamma's shape
    x = L.PnPoolBwdArgs()
    x.a, x.w, x.gamma, x.dout, x.saved, x.scratch = a.data_ptr(), w.data_ptr(), gamma.data_ptr(), dout.data_ptr(), \
        saved.data_ptr(), scratch.data_ptr()
    x.da, x.dw, x.db, x.dgamma, x.dbeta = _p(da), dw.data_ptr(), db.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr()
    if rag is None:
        L.check(lib.pnpp_pn_pool_backward(C.byref(d), C.byref(x), _stream()))
    else:
        L.check(lib.pnpp_pn_pool_backward_ragged(C.byref(d), C.byref(x), rag.offs_dev.data_ptr(), rag.M_total, _stream()))
    return da, returned


def _pn_rows(rag, B: int, N: int) -> int:
    return B * N if rag is None else rag.M_total


def _pn_packed(lengths, B: int, N: int, device):
    """lengths=None -> None (the uniform code path, untouched); anything else -> the batch's PackedLengths"""
    return None if lengths is None else packed_lengths(lengths, B, N, device)


class _PnPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, w, b, gamma, beta, cfg):
        B, N, relu, training, eps, momentum, rm, rv, nbt, rag = cfg
        a, w, b = _f32(a, "a"), _f32(w, "conv weight"), _f32(b, "conv bias")
        gamma, beta = _f32(gamma, "bn weight"), _f32(beta, "bn bias")
        if a.dim() != 2 or a.shape[0] != _pn_rows(rag, B, N):
            raise ValueError(f"pn_pool: expected ({_pn_rows(rag, B, N)}, K) rows, got {tuple(a.shape)}")
        K, Cc = a.shape[1], w.shape[0]
        if w.numel() != Cc * K:
            raise ValueError(f"pn_pool: weight {tuple(w.shape)} does not map {K} inputs")
        d = _pn_pool_desc(B, N, K, Cc, relu, training, eps, momentum)
        out, saved = _pn_pool_forward_call(d, a, w, b, gamma, beta, rm, rv, nbt, rag)
        ctx.desc, ctx.rag = d, rag
        ctx.save_for_backward(a, w, gamma, saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        a, w, gamma, saved = ctx.saved_tensors
        da, grads = _pn_pool_backward_call(ctx.desc, a, w, gamma, _f32(dout, "dout"), saved, ctx.rag, ctx.needs_input_grad[0], None)
        return (da, *grads, None)


def pn_pool(a: torch.Tensor, B: int, N: int, conv, bn, relu: bool, training: bool, lengths=None) -> torch.Tensor:
    """max over each cloud's N rows of act(bn(conv(a))): a (B*N, K) rows, conv a 1x1 nn.Conv1d, bn its nn.BatchNorm1d (running
    statistics updated in place when training).  Returns (B, C).  Keeps O(B*C + K*K) for the backward pass, not (B*N) x C.
    lengths (B,) (pnpp_hip.lengths.packed_lengths): a holds the sum(lengths) PACKED valid rows of a ragged batch padded to N; the
    statistics run over those rows, each cloud's max over its own."""
    nbt = _nbt(bn) if training else None
    cfg = (int(B), int(N), bool(relu), bool(training), bn.eps, _bn_momentum(bn), bn.running_mean, bn.running_var, nbt,
           _pn_packed(lengths, int(B), int(N), a.device))
    return _PnPool.apply(a, conv.weight, conv.bias, bn.weight, bn.bias, cfg)


class _PnTransform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, k, ldy, rag, BN):
        _need_gpu(x, "x")
        if x.dtype != torch.float32:
            raise TypeError(f"x must be float32, got {x.dtype}")
        # rag None: x (B, N, D) -> (B*N, ldy) rows.  Ragged: x (B, N, D) padded, read in place, or (M_total, D) packed rows (the
        # padded geometry is BN then) -> (M_total, ldy) packed rows
        packed = rag is not None and x.dim() == 2
        if packed:
            B, N = BN
            x = x.contiguous()
            if x.shape[0] != rag.M_total:
                raise ValueError(f"pn_transform: expected ({rag.M_total}, D) packed rows, got {tuple(x.shape)}")
            D, (sb, sn, sd) = x.shape[1], (0, x.stride(0), x.stride(1))
        else:
            if not (x.is_contiguous() or x.transpose(1, 2).is_contiguous()):
                x = x.contiguous()
            if rag is not None and tuple(x.shape[:2]) != tuple(BN):
                raise ValueError(f"pn_transform: expected a ({BN[0]}, {BN[1]}, D) input, got {tuple(x.shape)}")
            (B, N, D), (sb, sn, sd) = x.shape, x.stride()
        if t is not None:
            t = _f32(t, "transform")
            if tuple(t.shape) != (B, k, k):
                raise ValueError(f"pn_transform: transform {tuple(t.shape)} is not ({B}, {k}, {k})")
        y = torch.empty(_pn_rows(rag, B, N), ldy, device=x.device, dtype=torch.float32)
        if rag is None:
            L.check(L.lib().pnpp_pn_transform(x.data_ptr(), sb, sn, sd, _p(t), B, N, D, k, ldy, y.data_ptr(), _stream()))
        else:
            L.check(L.lib().pnpp_pn_transform_ragged(x.data_ptr(), int(packed), sb, sn, sd, _p(t), rag.offs_dev.data_ptr(), B, N, D, k, ldy,
                                                     y.data_ptr(), _stream()))
        ctx.k, ctx.ldy, ctx.has_t, ctx.rag = k, ldy, t is not None, rag
        ctx.geom = (packed, B, N, D, sb, sn, sd)
        ctx.save_for_backward(x, t if t is not None else x.new_empty(0))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, t = ctx.saved_tensors
        t = t if ctx.has_t else None
        dy = _f32(dy, "dy")
        packed, B, N, D, sb, sn, sd = ctx.geom
        # every element of dx is written: the padding rows of a padded ragged input get exact zeros
        dx = torch.empty_strided(x.shape, x.stride(), device=x.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dt = torch.empty_like(t) if (t is not None and ctx.needs_input_grad[1]) else None
        if dx is None and dt is None:
            return None, None, None, None, None, None
        if ctx.rag is None:
            L.check(L.lib().pnpp_pn_transform_bwd(x.data_ptr(), sb, sn, sd, _p(t), dy.data_ptr(), B, N, D, ctx.k, ctx.ldy, _p(dx), _p(dt),
                                                  _stream()))
        else:
            L.check(L.lib().pnpp_pn_transform_bwd_ragged(x.data_ptr(), int(packed), sb, sn, sd, _p(t), dy.data_ptr(),
                                                         ctx.rag.offs_dev.data_ptr(), B, N, D, ctx.k, ctx.ldy, _p(dx), _p(dt), _stream()))
        return dx, dt, None, None, None, None


def pn_transform(x: torch.Tensor, t: Optional[torch.Tensor], ldy: int, lengths=None, B: Optional[int] = None,
                 N: Optional[int] = None) -> torch.Tensor:
    """x (B, N, D) -- any dense layout, e.g. the transpose of a (B, D, N) input, read in place -- times the per-cloud transform
    t (B, k, k) on its first k columns, the other D - k columns passed through, zero columns up to ldy: (B*N, ldy) rows.
    t None: the strided copy into (B*N, ldy) rows alone.
    lengths (B,): the batch is ragged, cloud b its first lengths[b] points.  The result is the (sum(lengths), ldy) PACKED rows, cloud
    after cloud; the padding of x is never read and its gradient there is an exact zero.  x may also be (sum(lengths), D) packed
    rows already (a later layer of the same batch): pass the padded geometry as B and N then."""
    k = t.shape[-1] if t is not None else 0
    if lengths is None:
        return _PnTransform.apply(x, t, k, int(ldy), None, None)
    if x.dim() == 3:
        B, N = x.shape[0], x.shape[1]
    elif B is None or N is None:
        raise ValueError("pn_transform: packed rows need the padded geometry B and N")
    return _PnTransform.apply(x, t, k, int(ldy), packed_lengths(lengths, int(B), int(N), x.device), (int(B), int(N)))


class _PnRegularizer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        t = _f32(t, "trans")
        if t.dim() != 3 or t.shape[1] != t.shape[2]:
            raise ValueError(f"feature_transform_regularizer: expected (B, k, k), got {tuple(t.shape)}")
        B, k = t.shape[0], t.shape[1]
        norms = torch.empty(B, device=t.device, dtype=torch.float64)
        out = torch.empty((), device=t.device, dtype=torch.float32)
        L.check(L.lib().pnpp_pn_regularizer(t.data_ptr(), B, k, norms.data_ptr(), out.data_ptr(), _stream()))
        ctx.save_for_backward(t, norms)
        return out

    @staticmethod
    def backward(ctx, g):
        t, norms = ctx.saved_tensors
        g = _f32(g, "grad")
        dt = torch.empty_like(t)
        L.check(L.lib().pnpp_pn_regularizer_bwd(t.data_ptr(), norms.data_ptr(), g.data_ptr(), t.shape[0], t.shape[1], dt.data_ptr(),
                                                _stream()))
        return dt


def feature_transform_regularizer(trans: torch.Tensor) -> torch.Tensor:
    """mean_b ||T_b T_b^T - I||_F of (B, k, k) transforms (PointNetDemo.py's feature_transform_reguliarzer), a 0-d tensor;
    forward and backward on the device."""
    return _PnRegularizer.apply(trans)


class _PnAddIdentity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        x = _f32(x, "x")
        B = x.shape[0]
        if x.numel() != B * k * k:
            raise ValueError(f"pn_add_identity: {tuple(x.shape)} is not ({B}, {k * k})")
        y = torch.empty(B, k, k, device=x.device, dtype=torch.float32)
        L.check(L.lib().pnpp_pn_add_identity(x.data_ptr(), B, k, y.data_ptr(), _stream()))
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy.reshape(ctx.shape), None


def pn_add_identity(x: torch.Tensor, k: int) -> torch.Tensor:
    """(B, k*k) -> (B, k, k) + I: the T-Nets' `fc3(x) + iden`."""
    return _PnAddIdentity.apply(x, int(k))


class _PnConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, pf, N, rag, pf_padded):
        g, pf = _f32(g, "global feature"), _f32(pf, "point features")
        B, C1 = g.shape
        C2 = pf.shape[1]
        rows = B * N if (rag is None or pf_padded) else rag.M_total
        if pf.shape[0] != rows:
            raise ValueError(f"pn_concat: point features {tuple(pf.shape)} are not ({rows}, C)")
        out = torch.empty(B, C1 + C2, N, device=g.device, dtype=torch.float32)
        if rag is None:
            L.check(L.lib().pnpp_pn_concat(g.data_ptr(), pf.data_ptr(), B, N, C1, C2, out.data_ptr(), _stream()))
        else:
            L.check(L.lib().pnpp_pn_concat_ragged(g.data_ptr(), pf.data_ptr(), int(pf_padded), rag.offs_dev.data_ptr(), B, N, C1, C2,
                                                  out.data_ptr(), _stream()))
        ctx.dims, ctx.rag, ctx.pf_padded = (B, N, C1, C2), rag, pf_padded
        return out

    @staticmethod
    def backward(ctx, dout):
        B, N, C1, C2 = ctx.dims
        dout = _f32(dout, "dout")
        dg = torch.empty(B, C1, device=dout.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        rag = ctx.rag
        if rag is not None and ctx.pf_padded and ctx.needs_input_grad[1]:
            raise RuntimeError("pn_concat: padded point features are a forward-only input")
        dpf = torch.empty(_pn_rows(rag, B, N), C2, device=dout.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        if dg is None and dpf is None:
            return None, None, None, None, None
        if rag is None:
            L.check(L.lib().pnpp_pn_concat_bwd(dout.data_ptr(), B, N, C1, C2, _p(dg), _p(dpf), _stream()))
        else:
            L.check(L.lib().pnpp_pn_concat_bwd_ragged(dout.data_ptr(), rag.offs_dev.data_ptr(), B, N, C1, C2, _p(dg), _p(dpf), _stream()))
        return dg, dpf, None, None, None


def pn_concat(g: torch.Tensor, pf: torch.Tensor, N: int, lengths=None, pf_padded: bool = False) -> torch.Tensor:
    """cat([g (B, C1) repeated over the N points, pf (B*N, C2) rows transposed], 1) -> (B, C1 + C2, N).
    lengths (B,): pf holds the (sum(lengths), C2) packed rows of a ragged batch (pf_padded: the padded B*N rows, forward only); the
    columns n >= lengths[b] of the output are exact zeros and the incoming gradient there is not read."""
    rag = None if lengths is None else packed_lengths(lengths, g.shape[0], int(N), g.device, need_total=not pf_padded)
    return _PnConcat.apply(g, pf, int(N), rag, bool(pf_padded))


class _PnBnRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, cfg):
        training, eps, momentum, rm, rv, nbt = cfg
        x, gamma, beta = _f32(x, "x"), _f32(gamma, "bn weight"), _f32(beta, "bn bias")
        M, Cc = x.shape
        mean, istd = torch.empty(Cc, device=x.device, dtype=torch.float32), torch.empty(Cc, device=x.device, dtype=torch.float32)
        y = torch.empty_like(x)
        L.check(L.lib().pnpp_pn_bn_relu(x.data_ptr(), M, Cc, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), _p(nbt),
                                        int(training), float(eps), float(momentum), mean.data_ptr(), istd.data_ptr(), y.data_ptr(),
                                        _stream()))
        ctx.training = bool(training)
        ctx.save_for_backward(x, y, gamma, mean, istd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, mean, istd = ctx.saved_tensors
        dy = _f32(dy, "dy")
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        L.check(L.lib().pnpp_pn_bn_relu_bwd(x.data_ptr(), y.data_ptr(), dy.data_ptr(), x.shape[0], x.shape[1], gamma.data_ptr(),
                                            mean.data_ptr(), istd.data_ptr(), int(ctx.training), _p(dx), dgamma.data_ptr(),
                                            dbeta.data_ptr(), _stream()))
        return dx, dgamma, dbeta, None


def pn_bn_relu(x: torch.Tensor, bn, training: bool) -> torch.Tensor:
    """relu(bn(x)) for (M, C) rows with an nn.BatchNorm1d on its own (running statistics updated in place when training)."""
    nbt = _nbt(bn) if training else None
    return _PnBnRelu.apply(x, bn.weight, bn.bias, (bool(training), bn.eps, _bn_momentum(bn), bn.running_mean, bn.running_var, nbt))


# set to a list to receive, per narrow layer of a pn_trunk call, its (B*N, C) ReLU decisions (y > 0, on the host) in call order
pn_relu_tap: Optional[list] = None


class _PnTrunk(torch.autograd.Function):
    """Per-point layers (1x1 conv -> train/eval BatchNorm -> ReLU) followed by the pooled wide layer, as one autograd node that
    keeps only the input rows, each narrow layer's pre-BatchNorm output (its fc workspace) and the pooled layer's small workspace:
    the narrow layers' outputs are recomputed from their workspaces in the backward pass (pnpp_fc_recompute_output)."""

    @staticmethod
    def forward(ctx, rows, cfg, *params):
        B, N, nl, pool_relu, training, eps, mom, running, nbts, sinks, rag = cfg
        rows = _f32(rows, "rows")
        M = _pn_rows(rag, B, N)
        if rows.dim() != 2 or rows.shape[0] != M:
            raise ValueError(f"pn_trunk: expected ({M}, K) rows, got {tuple(rows.shape)}")
        if M <= 32:
            raise ValueError(f"pn_trunk: {B} clouds x {N} points = {M} point rows; the per-point layers need more than 32")
        x, descs, saveds = rows, [], []
        for l in range(nl):
            w, b, nw, nb = (_f32(t, "trunk parameter") for t in params[4 * l:4 * l + 4])
            d = _fc_desc(M, x.shape[1], w.shape[0], L.NORM_BATCH, 1, training, eps[l], mom[l], 1.0)
            y, saved, _ = _fc_forward_call(d, x, w, b, nw, nb, running[2 * l], running[2 * l + 1], nbts[l], None, None)
            if pn_relu_tap is not None:
                pn_relu_tap.append((y > 0).cpu())
            descs.append(d)
            saveds.append(saved)
            x = y
        w, b, nw, nb = (_f32(t, "pooled layer parameter") for t in params[4 * nl:4 * nl + 4])
        pd = _pn_pool_desc(B, N, x.shape[1], w.shape[0], pool_relu, training, eps[nl], mom[nl])
        out, psaved = _pn_pool_forward_call(pd, x, w, b, nw, nb, running[2 * nl], running[2 * nl + 1], nbts[nl], rag)
        ctx.descs, ctx.pdesc, ctx.sinks, ctx.nl, ctx.rag = descs, pd, sinks, nl, rag
        ctx.save_for_backward(rows, psaved, *saveds, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        nl, descs, pd = ctx.nl, ctx.descs, ctx.pdesc
        t = ctx.saved_tensors
        rows, psaved, saveds, params = t[0], t[1], t[2:2 + nl], t[2 + nl:]
        sinks = ctx.sinks or [None] * len(params)
        dout = _f32(dout, "dout")
        lib = L.lib()
        dev = rows.device
        ys = []
        for l in range(nl):   # the narrow layers' outputs, bit-identical to the forward pass's
            y = torch.empty(descs[l].M, descs[l].N, device=dev, dtype=torch.float32)
            L.check(lib.pnpp_fc_recompute_output(C.byref(descs[l]), saveds[l].data_ptr(), None, y.data_ptr(), _stream()))
            ys.append(y)
        grads = [None] * len(params)
        w, _, nw, _ = params[4 * nl:4 * nl + 4]
        dy, grads[4 * nl:] = _pn_pool_backward_call(pd, ys[-1] if nl else rows, w, nw, dout, psaved, ctx.rag,
                                                    nl or ctx.needs_input_grad[0], sinks[4 * nl:])
        for l in reversed(range(nl)):
            w, b, nw, nb = params[4 * l:4 * l + 4]
            dy, grads[4 * l:4 * l + 4] = _fc_backward_call(descs[l], ys[l - 1] if l else rows, w, b, nw, nb, None, dy, saveds[l],
                                                            l or ctx.needs_input_grad[0], sinks[4 * l:4 * l + 4])
        return (dy, None, *grads)


def pn_trunk(rows: torch.Tensor, B: int, N: int, layers, pooled, pool_relu: bool, training: bool, lengths=None) -> torch.Tensor:
    """(B*N, K) point rows -> relu(bn(conv)) for each (conv, bn) of `layers` (0 - 2 of them, 1x1 nn.Conv1d + nn.BatchNorm1d) ->
    the pooled wide layer `pooled` = (conv, bn) with its max over each cloud's N points: (B, C).  Keeps for the backward pass
    only the rows, the narrow layers' pre-BatchNorm outputs and O(B*C + K^2) for the pooled layer.
    lengths (B,): rows are the M = sum(lengths) PACKED valid rows of a ragged batch padded to N (pn_transform(..., lengths=)); every
    BatchNorm takes its statistics over those M rows, each cloud's max runs over its own, and M > 32 takes the place of B*N > 32."""
    rag = _pn_packed(lengths, int(B), int(N), rows.device)
    if rag is not None and rag.M_total <= 32:
        raise ValueError(f"pn_trunk: the lengths of the {B} clouds sum to {rag.M_total} point rows; the per-point layers need more than 32")
    params, running, nbts, eps, mom = [], [], [], [], []
    for conv, bn in list(layers) + [pooled]:
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
        running += [bn.running_mean, bn.running_var]
        nbts.append(_nbt(bn) if training else None)
        eps.append(bn.eps)
        mom.append(_bn_momentum(bn))
    sinks = [grad_sink(p) for p in params]
    cfg = (int(B), int(N), len(layers), bool(pool_relu), bool(training), eps, mom, running, nbts,
           sinks if any(s is not None for s in sinks) else None, rag)
    return _PnTrunk.apply(rows, cfg, *params)
