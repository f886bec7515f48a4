"""numpy float64 restatement of the surface-normal definition (include/pnpp_hip.h: pnpp_estimate_normals), the seeded cloud families and
the case table of tests/test_gpu_normals.py.  The eigen-solver is numpy.linalg.eigh, independent of the kernel's cyclic Jacobi.

normals_ref takes the neighbour lists as an argument: the device lists (held to the oracle by the index tests and, in the normals
tests, bit-equal to ops.knn) are what it is fed, so what it checks is the covariance, the eigenvector, the sign and the curvature."""
import numpy as np

ILL_GAP = 1e-3      # (l1 - l0) / l2 below this: the normal's direction is ill-conditioned, a point the gates leave out
SIGN_TIE = 1e-4     # |n . (p - r)| below this fraction of |p - r|: the orientation is a tie
CANON_TIE = 1e-6    # mode "none": the two largest |components| of n closer than this (the normal is good to 2.5e-7): the canonical sign is a tie

ANGLE_GATE = 2.5e-7   # rad: float32 rounding of a unit vector (<= 1.03e-7 = sqrt(3) * 2^-24) + a float64 solve at gap >= 1e-3 (~1e-13)
NORM_GATE = 2e-7
CURV_GATE = 6e-8      # one float32 rounding of a value <= 1/3 (half an ulp there is 1.5e-8)
MAX_EXCLUDED = 0.02


def normals_ref(xyz, idx, ref=None, mode="none"):
    """xyz (B, N, 3) float32, idx (B, N, k) integer neighbour lists, ref (B, 3) float32 reference points, mode "none" / "away" / "toward"
    -> (normals (B, N, 3) float64, curvature (B, N) float64, ill (B, N) bool, sign_tie (B, N) bool)."""
    assert mode in ("none", "away", "toward")
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 3
    B, N, _ = xyz.shape
    idx = np.asarray(idx).astype(np.int64)
    k = idx.shape[2]
    normals, curv = np.zeros((B, N, 3)), np.zeros((B, N))
    ill, tie = np.zeros((B, N), bool), np.zeros((B, N), bool)
    for b in range(B):
        P = xyz[b].astype(np.float64)
        d = P[idx[b]] - P[:, None, :]                                  # (N, k, 3)
        m = d.sum(axis=1) / k
        C = np.einsum("nki,nkj->nij", d, d) / k - m[:, :, None] * m[:, None, :]
        C = 0.5 * (C + np.transpose(C, (0, 2, 1)))
        w, v = np.linalg.eigh(C)                                       # ascending
        trace = C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]
        flat = trace <= 0.0
        n = v[:, :, 0].copy()
        big = np.argmax(np.abs(n), axis=1)                             # the first maximum: the lowest index among equal magnitudes
        n[n[np.arange(N), big] < 0.0] *= -1.0
        a = np.sort(np.abs(n), axis=1)
        t = np.zeros(N, bool)
        if mode == "none":
            t = (a[:, 2] - a[:, 1]) < CANON_TIE
        else:
            r = np.asarray(ref)[b].astype(np.float64)
            pr = P - r[None, :]
            s = (n[:, 0] * pr[:, 0] + n[:, 1] * pr[:, 1]) + n[:, 2] * pr[:, 2]
            n[(s < 0.0) if mode == "away" else (s > 0.0)] *= -1.0
            t = np.abs(s) < SIGN_TIE * np.linalg.norm(pr, axis=1)
        den = w.sum(axis=1)
        c = np.where(den > 0.0, np.maximum(w[:, 0], 0.0) / np.where(den > 0.0, den, 1.0), 0.0)
        n[flat], c[flat] = 0.0, 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = (w[:, 1] - w[:, 0]) / w[:, 2]
        normals[b], curv[b] = n, c
        ill[b] = flat | ~(gap >= ILL_GAP)
        tie[b] = t & ~flat
    return normals, curv, ill, tie


def knn_bruteforce(xyz, k):
    """Neighbour lists for the CPU checks of the restatement (float64 distances, ascending (distance, index)): NOT the device's bit-exact
    float32 keys -- the GPU tests feed normals_ref the device lists."""
    xyz = np.asarray(xyz, np.float64)
    out = np.zeros(xyz.shape[:2] + (k,), np.int64)
    for b in range(xyz.shape[0]):
        d = ((xyz[b][:, None, :] - xyz[b][None, :, :]) ** 2).sum(-1)
        out[b] = np.lexsort((np.broadcast_to(np.arange(d.shape[1]), d.shape), d), axis=1)[:, :k]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded cloud families, all float32
# ---------------------------------------------------------------------------------------------------------------------------------
def cube(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def sphere(n, seed):
    """A unit sphere shell with 1 % radial noise."""
    g = np.random.default_rng(seed)
    v = g.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (1.0 + 0.01 * g.standard_normal((n, 1)))).astype(np.float32)


def box(n, seed):
    """The six faces of a 1 x 0.5 x 0.3 box translated by (100, -50, 7): float32 coordinates whose differences need float64."""
    g = np.random.default_rng(seed)
    size = np.array([1.0, 0.5, 0.3])
    p = g.random((n, 3)) * size
    face = g.integers(0, 6, n)
    axis, side = face // 2, face % 2
    p[np.arange(n), axis] = side * size[axis]
    return (p + np.array([100.0, -50.0, 7.0])).astype(np.float32)


def plane(n, seed):
    """The exact plane z = 0.25."""
    p = np.random.default_rng(seed).random((n, 3))
    p[:, 2] = 0.25
    return p.astype(np.float32)


def copies(n, seed, ncopy=40):
    """n points of the cube family, the first ncopy of them one and the same point."""
    p = cube(n, seed)
    p[:ncopy] = p[0]
    return p


FAMILIES = {"cube": cube, "sphere": sphere, "box": box, "plane": plane, "copies": copies}


def batch(families, n, seed):
    """(B, n, 3) float32: cloud b from families[b], seeded seed + b."""
    return np.stack([FAMILIES[f](n, seed + b) for b, f in enumerate(families)])


# name -> families (one per cloud), N, k, orient ("centroid", None, or a viewpoint), what the shape exercises
CASES = {
    "n64_k8": dict(families=("cube", "box"), N=64, k=8, orient="centroid"),             # one partial lane chunk, several passes per workgroup
    "n200_k16": dict(families=("sphere", "box"), N=200, k=16, orient="centroid"),       # N no multiple of 64, nor of the queries per workgroup
    "n64_k3_cube": dict(families=("cube",), N=64, k=3, orient="centroid"),              # the minimum k: a rank-2 covariance
    "n300_k64": dict(families=("box",), N=300, k=64, orient="centroid"),                # a full first list slot per lane
    "n300_k100": dict(families=("sphere",), N=300, k=100, orient="centroid"),           # the second list slot per lane, lane + 64
    "n1024_k16": dict(families=("box",), N=1024, k=16, orient="centroid"),              # exactly one tile
    "n1100_k16": dict(families=("cube", "sphere"), N=1100, k=16, orient="centroid"),    # two tiles: neighbours from global memory, qpw = 1
    "n200_k16_none": dict(families=("cube", "sphere"), N=200, k=16, orient=None),       # the canonical sign alone
    "n200_k16_view": dict(families=("box", "cube"), N=200, k=16, orient=(103.0, -47.0, 11.0)),   # mode "toward"
}
SEED = 20260
