"""CPU restatement (numpy) of csrc/view_kernels.hip: the per-cloud angles in float64 rounded to float32 once, every float32 step an IEEE
basic operation in the kernel's order, integer cells, an order-free depth-buffer maximum and a stable mask.  Test infrastructure; the
Philox words are oracle.sampler's."""
import numpy as np

from oracle.sampler import philox4x32_10

F32 = np.float32
K_ANGLE = 2.0 * np.pi / 4294967296.0          # exact: a power-of-two division
CLOUD_N = 0xFFFFFFFF
STREAM_BASE = 1 << 62
RESAMPLE_BASE = STREAM_BASE | (1 << 61)
ELEVATION = (-np.pi / 6, np.pi / 3)


def _words(n, slot, seed, stream_id):
    return philox4x32_10(n, slot, stream_id & 0xFFFFFFFF, (stream_id >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def cloud_words(seed, stream_id, B):
    return _words(np.uint64(CLOUD_N), np.arange(B, dtype=np.uint64), seed, stream_id)


def drawn_angles(seed, stream_id, B, elevation=ELEVATION):
    """-> (phi, eps) (B,) float64: azimuth w0 2 pi / 2^32, elevation lo + (hi - lo) w1 / 2^32 with lo, hi as float32."""
    w = cloud_words(seed, stream_id, B)
    lo, hi = np.float64(F32(elevation[0])), np.float64(F32(elevation[1]))
    return w[0].astype(np.float64) * K_ANGLE, lo + (hi - lo) * (w[1].astype(np.float64) * (1.0 / 4294967296.0))


def angles_of_dirs(dirs):
    """(B,3) float32 directions towards the viewer -> (ca, sa, ce, se) float64, the kernel's normalisation."""
    g = np.asarray(dirs, F32).astype(np.float64)
    ca, sa, ce, se = np.ones(len(g)), np.zeros(len(g)), np.ones(len(g)), np.zeros(len(g))
    for b, (x, y, z) in enumerate(g):
        ln = np.sqrt(x * x + y * y + z * z)
        if ln > 0 and np.isfinite(ln):
            nx, ny, nz = x / ln, y / ln, z / ln
            se[b], ce[b] = ny, np.sqrt(nx * nx + nz * nz)
            sa[b], ca[b] = (nx / ce[b], -nz / ce[b]) if ce[b] > 0 else (0.0, 1.0)
    return ca, sa, ce, se


def basis(ca, sa, ce, se):
    """Float64 cosines and sines -> v, r, u (B,3) float32: each rounded once, then the float32 products."""
    ca, sa, ce, se = (np.asarray(t, np.float64).astype(F32) for t in (ca, sa, ce, se))
    z = np.zeros_like(ca)
    v = np.stack([ce * sa, se, -(ce * ca)], 1).astype(F32)
    r = np.stack([ca, z, sa], 1).astype(F32)
    u = np.stack([-(se * sa), ce, se * ca], 1).astype(F32)
    return v, r, u


def basis_of(seed, stream_id, B, elevation=ELEVATION, view_dirs=None, angles=None, params=None):
    """The separate float64 computation of (v, r, u).  With the device's params it is held to one float32 spacing of the device's
    v, azimuth and elevation, and the device's own v is what the restatement then projects on."""
    if view_dirs is not None:
        cs = angles_of_dirs(view_dirs)
        phi, eps = np.arctan2(cs[1], cs[0]), np.arctan2(cs[3], cs[2])
    else:
        if angles is not None:
            a = np.asarray(angles, F32).astype(np.float64)
            phi, eps = a[:, 0], a[:, 1]
        else:
            phi, eps = drawn_angles(seed, stream_id, B, elevation)
        cs = (np.cos(phi), np.sin(phi), np.cos(eps), np.sin(eps))
    v, r, u = basis(*cs)
    if params is not None:
        p = np.asarray(params, F32)
        assert (np.abs(p[:, :3].astype(np.float64) - v) <= np.spacing(np.maximum(np.abs(v), F32(2.0 ** -24)))).all(), (p[:, :3], v)
        for got, want in ((p[:, 3], phi), (p[:, 4], eps)):
            assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.maximum(np.abs(want.astype(F32)), F32(2.0 ** -24)))).all()
        v = p[:, :3].copy()
    return v, r, u


def dot3(p, e):
    """fl(fl(fl(x e_x) + fl(y e_y)) + fl(z e_z)); p (n,3) float32, e (3,) float32 (numpy rounds after every operation)."""
    p, e = np.asarray(p, F32), np.asarray(e, F32)
    return ((p[:, 0] * e[0]).astype(F32) + (p[:, 1] * e[1]).astype(F32)).astype(F32) + (p[:, 2] * e[2]).astype(F32)


def _key(d):
    b = np.asarray(d, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def cells(a, amin, cell, G):
    if not cell > 0:
        return np.zeros(len(a), np.int64)
    with np.errstate(all="ignore"):
        q = np.floor(((a - amin).astype(F32) / cell).astype(F32))
        return np.maximum(F32(0), np.minimum(q, F32(G - 1))).astype(np.int64)


def visible(pts, v, r, u, G, splat, thickness):
    """One cloud's valid rows (n,3) -> (mask (n,) bool, cell float32): projection, extent, depth buffer, test."""
    pts = np.asarray(pts, F32)
    d, a, t = dot3(pts, v), dot3(pts, r), dot3(pts, u)
    amin, amax, tmin, tmax = (F32(x + F32(0.0)) for x in (a.min(), a.max(), t.min(), t.max()))
    ext = max(F32(amax - amin), F32(tmax - tmin))
    cell = F32(ext / F32(G))
    ia, it = cells(a, amin, cell, G), cells(t, tmin, cell, G)
    z = np.zeros((G, G), np.uint32)
    key = _key(d)
    for di in range(-splat, splat + 1):
        for dj in range(-splat, splat + 1):
            i, j = ia + di, it + dj
            ok = (i >= 0) & (i < G) & (j >= 0) & (j < G)
            np.maximum.at(z, (i[ok], j[ok]), key[ok])
    with np.errstate(all="ignore"):
        mask = (_unkey(z[ia, it]) - d).astype(F32) <= F32(F32(thickness) * ext)
    return mask, cell


def thin(mask, b, seed, stream_id, drop):
    """drop > 0: a visible point survives iff word 0 of its own Philox words >= fl64(drop w2), w2 the cloud's third word."""
    if not drop > 0:
        return mask
    w2 = _words(np.uint64(CLOUD_N), np.uint64(b), seed, stream_id)[2]
    thresh = np.float64(F32(drop)) * np.float64(w2)
    own = _words(np.arange(len(mask), dtype=np.uint64), np.uint64(b), seed, stream_id)[0]
    return mask & (own.astype(np.float64) >= thresh)


def resolution(N):
    import math
    return min(128, max(1, math.isqrt(max(N, 1) - 1) + 1))


def view(xyz, v, r, u, seed=0, stream_id=0, lengths=None, G=None, splat=1, thickness=0.1, drop=0.0, min_keep=1):
    """The kernel's outputs for given per-cloud v, r, u (B,3) float32: -> (xyz_out (B,N,C), lengths_out (B,) int32, index (B,N) int32,
    cell (B,) float32, passed (B,) bool).  Rows at or beyond lengths[b] (clamped to 1..N) are never looked at."""
    xyz = np.asarray(xyz, F32)
    B, N, _ = xyz.shape
    G = resolution(N) if G is None else G
    out, idx = np.zeros_like(xyz), np.full((B, N), -1, np.int32)
    kept, cell, passed = np.zeros(B, np.int32), np.zeros(B, F32), np.zeros(B, bool)
    for b in range(B):
        nv = N if lengths is None else min(max(int(lengths[b]), 1), N)
        mask, cell[b] = visible(xyz[b, :nv, :3], v[b], r[b], u[b], G, splat, thickness)
        mask = thin(mask, b, seed, stream_id, drop)
        if mask.sum() < min_keep:
            mask, passed[b] = np.ones(nv, bool), True
        src = np.nonzero(mask)[0]
        kept[b] = len(src)
        out[b, :len(src)] = xyz[b, src]
        idx[b, :len(src)] = src
    return out, kept, idx, cell, passed
