"""CPU restatement (numpy) of csrc/augment_kernels.hip: the per-cloud parameters and the jitter in float64 rounded to float32 once,
every float32 step an IEEE basic operation in the kernel's order.  Test infrastructure; the Philox words are oracle.sampler's."""
import numpy as np

from oracle.sampler import philox4x32_10

F32 = np.float32
TWO_PI = 2.0 * np.pi
K_ANGLE = TWO_PI / 4294967296.0          # exact: a power-of-two division
CLOUD_N = 0xFFFFFFFF
STREAM_BASE = 1 << 63


def _words(n, slot, seed, stream_id):
    return philox4x32_10(n, slot, stream_id & 0xFFFFFFFF, (stream_id >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def theta(seed, stream_id, B):
    """(B,) float64 yaw angles: w0 of the cloud's words times 2 pi / 2^32."""
    w = _words(np.uint64(CLOUD_N), np.arange(B, dtype=np.uint64), seed, stream_id)
    return w[0].astype(np.float64) * K_ANGLE


def cloud_params(seed, stream_id, B, yaw=True, scale=None):
    """-> (theta (B,) f64, c, s, scale (B,) f32) as the kernel derives them."""
    w = _words(np.uint64(CLOUD_N), np.arange(B, dtype=np.uint64), seed, stream_id)
    th = w[0].astype(np.float64) * K_ANGLE if yaw else np.zeros(B)
    c = np.cos(th).astype(F32) if yaw else np.ones(B, F32)
    s = np.sin(th).astype(F32) if yaw else np.zeros(B, F32)
    if scale is None:
        sc = np.ones(B, F32)
    else:
        lo, hi = np.float64(F32(scale[0])), np.float64(F32(scale[1]))
        sc = (lo + (hi - lo) * (w[1].astype(np.float64) * (1.0 / 4294967296.0))).astype(F32)
    return th, c, s, sc


def rotate_f32(c, s, x, z):
    """x' = fl(fl(c x) + fl(s z)), z' = fl(fl(c z) - fl(s x)); all arrays float32 (numpy rounds after every operation)."""
    c, s, x, z = (np.asarray(v, F32) for v in (c, s, x, z))
    return (c * x).astype(F32) + (s * z).astype(F32), (c * z).astype(F32) - (s * x).astype(F32)


def jitter(seed, stream_id, B, N, sigma, clip):
    """(B, N, 3) float32: Box-Muller in float64 from each point's four words, clamped, rounded once."""
    w = _words(np.arange(N, dtype=np.uint64)[None, :], np.arange(B, dtype=np.uint64)[:, None], seed, stream_id)
    w = [v.astype(np.float64) for v in w]

    def pair(wa, wb):
        r = np.sqrt(-2.0 * np.log((wa + 1.0) * (1.0 / 4294967296.0)))
        return r * np.cos(wb * K_ANGLE), r * np.sin(wb * K_ANGLE)

    z0, z1 = pair(w[0], w[1])
    z2, _ = pair(w[2], w[3])
    sg, cl = np.float64(F32(sigma)), np.float64(F32(clip))
    return np.clip(sg * np.stack([z0, z1, z2], -1), -cl, cl).astype(F32)


def points(xyz, c, s, scale, lengths=None, yaw=True, use_scale=False, jit=None):
    """The kernel's rows for given per-cloud c, s, scale (B,) float32: rotate, then scale, then add jitter (B,N,3) float32; normals
    (columns 3..5) are rotated only; rows n >= lengths[b] are the input's."""
    xyz = np.asarray(xyz, F32)
    out = xyz.copy()
    cb, sb = np.asarray(c, F32)[:, None], np.asarray(s, F32)[:, None]
    if yaw:
        out[..., 0], out[..., 2] = rotate_f32(cb, sb, xyz[..., 0], xyz[..., 2])
        if xyz.shape[-1] == 6:
            out[..., 3], out[..., 5] = rotate_f32(cb, sb, xyz[..., 3], xyz[..., 5])
    if use_scale:
        out[..., :3] = out[..., :3] * np.asarray(scale, F32)[:, None, None]
    if jit is not None:
        out[..., :3] = out[..., :3] + jit
    if lengths is not None:
        pad = np.arange(xyz.shape[1])[None, :] >= np.asarray(lengths)[:, None]
        out[pad] = xyz[pad]
    return out


def shift_angles(mu, th):
    """mu' = (float32) wrap(float64(mu) - theta): one conditional + 2 pi; th broadcasts from (B,) over the trailing dims of mu."""
    mu = np.asarray(mu, F32)
    v = mu.astype(np.float64) - np.asarray(th, np.float64).reshape((-1,) + (1,) * (mu.ndim - 1))
    return np.where(v <= -np.pi, v + TWO_PI, v).astype(F32)


def vm_table(vm, th, counts=None):
    """(B,2) / (B,K,2) / (B,K,3): column 0 of the first counts[b] rows shifted, everything else copied."""
    vm = np.asarray(vm, F32)
    out = vm.copy()
    sh = shift_angles(vm[..., 0], th)
    if counts is not None and vm.ndim == 3:
        sh = np.where(np.arange(vm.shape[1])[None, :] < np.asarray(counts)[:, None], sh, vm[..., 0])
    out[..., 0] = sh
    return out


def axes(f, c, s):
    """(B,3) / (B,k,3) vectors rotated with the points' float32 arithmetic."""
    f = np.asarray(f, F32)
    out = f.copy()
    shape = (-1,) + (1,) * (f.ndim - 2)
    out[..., 0], out[..., 2] = rotate_f32(np.asarray(c, F32).reshape(shape), np.asarray(s, F32).reshape(shape), f[..., 0], f[..., 2])
    return out


def dir8(f, c, s, dirs8, yaw=True):
    """(B,3) forward axis -> (B,8): relu(dirs8 . R f) over its sequential sum; a zero sum gives 0.125 each."""
    f = axes(f, c, s) if yaw else np.asarray(f, F32)
    D = np.asarray(dirs8, F32)
    out = np.empty((f.shape[0], 8), F32)
    for b in range(f.shape[0]):
        r, tot = [], F32(0.0)
        for i in range(8):
            d = F32(F32(F32(D[i, 0] * f[b, 0]) + F32(D[i, 1] * f[b, 1])) + F32(D[i, 2] * f[b, 2]))
            r.append(d if d > 0 else F32(0.0))
            tot = F32(tot + r[-1])
        out[b] = [F32(0.125) if tot == 0 else F32(v / tot) for v in r]
    return out


def angular_distance(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % TWO_PI
    return np.minimum(d, TWO_PI - d)
