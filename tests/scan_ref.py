"""CPU restatement of the raw-scan preparation steps (include/pnpp_hip.h: pnpp_voxel_downsample, pnpp_outlier_statistic / _filter,
pnpp_normalize_clouds) in numpy: every float32 step is one IEEE operation on float32 values, in the order the header states, so the
device's rows, lengths and source rows can be held bit-equal to these.  The outlier step is fed neighbour lists -- its own brute-force
ones (knn_lists) or the device's."""
import numpy as np

F = np.float32
MAX_CELL = 1023


def valid_rows(lengths, b, N):
    return N if lengths is None else min(max(int(lengths[b]), 1), N)


def _compact(xyz, keep_rows, N):
    """rows of one cloud (N, C) and the kept source rows in order -> (out (N, C), kept, index (N,))"""
    out = np.zeros_like(xyz)
    idx = np.full(N, -1, dtype=np.int32)
    out[: len(keep_rows)] = xyz[keep_rows]
    idx[: len(keep_rows)] = keep_rows
    return out, len(keep_rows), idx


def bounds(p):
    """lo, hi per axis, a zero of either sign taken as +0"""
    return p.min(0) + F(0), p.max(0) + F(0)


def direct_dist(a, b):
    """(x-x')^2 + (y-y')^2 + (z-z')^2 in float32, summed in that order (csrc/exact_dist.h: direct_dist_exact)"""
    d = a - b
    s = d[..., 0] * d[..., 0]
    s = s + d[..., 1] * d[..., 1]
    return s + d[..., 2] * d[..., 2]


def voxel_cells(p, cell=None, grid=None):
    """p (n, 3) float32 -> (cell index per axis (n, 3) int64, 30-bit cell id (n,), d (n,) float32, h)"""
    with np.errstate(all="ignore"):
        lo, hi = bounds(p)
        h = F(cell) if cell is not None else (hi - lo).max() / F(grid)
        if not h > 0:
            h = F(1)
        q = np.floor((p - lo) / h)
        c = np.maximum(np.minimum(q, F(MAX_CELL if grid is None else grid - 1)), F(0))
        m = lo + (c + F(0.5)) * h
        d = direct_dist(p, m)
    ci = c.astype(np.int64)
    return ci, ci[:, 0] | (ci[:, 1] << 10) | (ci[:, 2] << 20), d.astype(F), h


def voxel_downsample(xyz, cell=None, grid=None, lengths=None):
    """-> (xyz' (B,N,C), lengths' (B,) int32, index (B,N) int32)"""
    assert (cell is None) != (grid is None)
    B, N, _ = xyz.shape
    out, lens, index = np.zeros_like(xyz), np.zeros(B, np.int32), np.zeros((B, N), np.int32)
    for b in range(B):
        Nv = valid_rows(lengths, b, N)
        _, ids, d, _ = voxel_cells(xyz[b, :Nv, :3], cell, grid)
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(Nv, dtype=np.uint64)
        order = np.lexsort((key, ids))                      # by cell, then by key
        first = np.ones(Nv, bool)
        first[1:] = ids[order][1:] != ids[order][:-1]
        out[b], lens[b], index[b] = _compact(xyz[b], np.sort(order[first]), N)
    return out, lens, index


def knn_lists(p, k1):
    """brute-force lists (n, k1) of the k1 nearest rows of every row of p, ascending (distance, row); the row itself comes first"""
    d = direct_dist(p[:, None, :], p[None, :, :])
    return np.argsort(d, axis=1, kind="stable")[:, :k1].astype(np.int32)


def outlier_statistic(p, lists, k):
    """p (n, 3) float32, lists (n, k + 1) -> s (n,) float64: the sum of sqrt((double) d) in list order over k + 1 entries, over k"""
    s = np.zeros(len(p), np.float64)
    for j in range(k + 1):
        s = s + np.sqrt(direct_dist(p, p[lists[:, j]]).astype(np.float64))
    return s / np.float64(k)


def remove_outliers(xyz, k, std_ratio, lengths=None, lists=None):
    """lists (B,N,k+1) or None (brute force per cloud) -> (xyz', lengths', index, stats (B,4) float64, statistic (B,N) float64)"""
    B, N, _ = xyz.shape
    out, lens, index = np.zeros_like(xyz), np.zeros(B, np.int32), np.zeros((B, N), np.int32)
    stats, stat = np.zeros((B, 4)), np.zeros((B, N))
    for b in range(B):
        Nv = valid_rows(lengths, b, N)
        if Nv <= k:
            out[b], lens[b], index[b] = _compact(xyz[b], np.arange(Nv), N)
            stats[b] = [0.0, 0.0, np.inf, Nv]
            if lists is not None:
                stat[b, :Nv] = outlier_statistic(xyz[b, :Nv, :3], np.clip(lists[b, :Nv], 0, Nv - 1), k)
            continue
        p = xyz[b, :Nv, :3]
        s = outlier_statistic(p, knn_lists(p, k + 1) if lists is None else lists[b, :Nv], k)
        mean = s.sum() / Nv
        std = np.sqrt(((s - mean) ** 2).sum() / Nv)
        thr = mean + std_ratio * std
        keep = np.nonzero(s <= thr)[0]
        out[b], lens[b], index[b] = _compact(xyz[b], keep, N)
        stats[b], stat[b, :Nv] = [mean, std, thr, len(keep)], s
    return out, lens, index, stats, stat


def normalize_clouds(xyz, lengths=None, centre="centroid", scale="sphere", given_centre=None):
    """-> (xyz', centre (B,3) float32, scale (B,) float32); given_centre (B,3): use these centres (the device's) instead"""
    B, N, _ = xyz.shape
    out, cs, rs = np.zeros_like(xyz), np.zeros((B, 3), F), np.ones(B, F)
    for b in range(B):
        Nv = valid_rows(lengths, b, N)
        p = xyz[b, :Nv, :3]
        with np.errstate(all="ignore"):
            lo, hi = bounds(p)
            c = np.zeros(3, F)
            if centre == "centroid":
                c = (p.astype(np.float64).sum(0) / Nv).astype(F)
            elif centre == "box":
                c = F(0.5) * (lo + hi)
            if given_centre is not None:
                c = given_centre[b].astype(F)
            q = p - c
            r = F(1)
            if scale == "sphere":
                sq = q[:, 0] * q[:, 0]
                sq = sq + q[:, 1] * q[:, 1]
                sq = sq + q[:, 2] * q[:, 2]
                r = np.sqrt(sq.max())
            elif scale == "box":
                r = F(0.5) * (hi - lo).max()
            if not r > 0:
                r = F(1)
            out[b, :Nv, :3] = q / r
        out[b, :Nv, 3:] = xyz[b, :Nv, 3:]
        cs[b], rs[b] = c, r
    return out, cs, rs


# ---- inputs shared by the CPU and GPU tests --------------------------------------------------------------------------------------
SURFACE_SCALE = np.array([1.0, 0.6, 0.3])


def surface(shape, n, rng):
    """n points on the surface of a unit sphere or of the cube [-1, 1]^3, scaled by (1, 0.6, 0.3); float64"""
    if shape == "sphere":
        v = rng.standard_normal((n, 3))
        p = v / np.linalg.norm(v, axis=1, keepdims=True)
    else:
        p = rng.uniform(-1.0, 1.0, (n, 3))
        face, side = rng.integers(0, 3, n), rng.integers(0, 2, n) * 2.0 - 1.0
        p[np.arange(n), face] = side
    return p * SURFACE_SCALE


def contaminated(shape, n, seed, fraction=0.05):
    """-> (xyz (n, 3) float32, injected (n,) bool): a surface with `fraction` of its rows replaced by uniform points in [-2, 2]^3"""
    rng = np.random.default_rng(seed)
    p = surface(shape, n, rng)
    injected = np.zeros(n, bool)
    injected[rng.choice(n, int(round(fraction * n)), replace=False)] = True
    p[injected] = rng.uniform(-2.0, 2.0, (int(injected.sum()), 3))
    return p.astype(F), injected
