"""numpy restatement of the yaw-symmetry definition (include/pnpp_hip.h: pnpp_yaw_profile, pnpp_yaw_symmetry), the seeded cloud families
and the case tables of tests/test_symmetry_cpu.py and tests/test_gpu_symmetry.py.

The definition, for one cloud of Nv points p_i, a centre c (float32; x and z are used) and a table of G float32 rows (cs, sn):
    centre     q_i = (p_i.x - c.x, p_i.y, p_i.z - c.z)
    rotate     x' = cs x + sn z, z' = cs z - sn x, y' = y                     (the order of the augmentation kernel)
    nearest    d[g,i] = min_j (dx dx + dy dy) + dz dz between rot_g(q_i) and q_j, the lowest j among equals (numpy's argmin)
    profile    D[g] = float32(sum_i float64(d[g,i]) / Nv)
    floor      nu = the same at the identity rotation (1, 0) with j != i; 0 when Nv = 1
    S, score   S[g] = D[g] + D[(G - g) % G], score = S / (2 nu)
    decision   bound = (2 nu) tol in float32; order 0 if S[g] <= bound for every g >= 1; else the largest m of `orders` with G % m == 0
               and S[k G / m] <= bound for k = 1..m-1; else 1
`profile(..., dtype=np.float32)` performs every step above as one float32 operation, in that order; `dtype=np.float64` performs the same
steps on the same float32 inputs in float64 (the judge of the arithmetic, tests/test_symmetry_cpu.py)."""
import math

import numpy as np
import torch

SEED = 20240611
ANGLE_BLOCK, TILE = 8, 1024     # the kernel's angle block and candidate tile: the CPU tests hold them equal to the library's constants
TOL, ORDERS = 1.3, (2, 3, 4, 6, 8)
QUERY_CHUNK = 256               # queries per numpy pass: N = 4097 stays a few MB


def grid_table(G):
    """(G, 2) float32 (cos, sin)(2 pi g / G) from float64, the multiples of a quarter turn exact."""
    a = 2.0 * np.pi * np.arange(G, dtype=np.float64) / G
    t = np.stack([np.cos(a), np.sin(a)], 1)
    quarter = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
    for g in range(G):
        if (4 * g) % G == 0:
            t[g] = quarter[4 * g // G]
    return t.astype(np.float32)


def _nearest(rx, rz, cx, cz, dy2, first, exclude_self):
    """min_j and argmin_j of (dx dx + dy2) + dz dz between queries (rx, rz) and candidates (cx, cz); dy2 (queries, candidates) does not
    depend on the rotation.  `first`: the index of the first query among the candidates, for the floor's j != i."""
    d = rx[:, None] - cx[None, :]
    np.multiply(d, d, out=d)
    d += dy2
    dz = rz[:, None] - cz[None, :]
    np.multiply(dz, dz, out=dz)
    d += dz
    r = np.arange(len(rx))
    if exclude_self:
        d[r, first + r] = np.inf
    j = np.argmin(d, axis=1)
    return d[r, j], j


def profile(xyz, centre, table, dtype=np.float32, nearest=False):
    """xyz (Nv, 3) float32, centre (3,) float32, table (G, 2) float32 -> D (G,) float32, nu float32 and, with nearest, d (G, Nv) in
    `dtype` and j (G, Nv) int32.  In float64 D and nu are returned unrounded."""
    xyz, centre, table = (np.asarray(v, np.float32).astype(dtype) for v in (xyz, centre, table))
    Nv, G = xyz.shape[0], table.shape[0]
    qx, qy, qz = xyz[:, 0] - centre[0], xyz[:, 1], xyz[:, 2] - centre[2]
    total = np.zeros(G + 1, np.float64)
    nd, ni = np.zeros((G, Nv), dtype), np.zeros((G, Nv), np.int32)
    one, zero = dtype(1.0), dtype(0.0)
    for s in range(0, Nv, QUERY_CHUNK):
        e = min(s + QUERY_CHUNK, Nv)
        x, z = qx[s:e], qz[s:e]
        dy2 = qy[s:e, None] - qy[None, :]
        np.multiply(dy2, dy2, out=dy2)
        for g in range(G):
            cs, sn = table[g, 0], table[g, 1]
            d, j = _nearest(cs * x + sn * z, cs * z - sn * x, qx, qz, dy2, s, False)
            total[g] += d.astype(np.float64).sum()
            if nearest:
                nd[g, s:e], ni[g, s:e] = d, j
        if Nv > 1:
            d, _ = _nearest(one * x + zero * z, one * z - zero * x, qx, qz, dy2, s, True)
            total[G] += d.astype(np.float64).sum()
    mean = total / Nv
    if dtype == np.float32:
        mean = mean.astype(np.float32)
    return (mean[:G], mean[G], nd, ni) if nearest else (mean[:G], mean[G])


def symmetric(D):
    G = len(D)
    return D + D[(G - np.arange(G)) % G]


def decide(D, nu, tol=TOL, orders=ORDERS, width=None):
    """The decision on a float32 profile -> (order, count, angles (width,) float32), width = max(orders) unless given."""
    D, nu = np.asarray(D, np.float32), np.float32(nu)
    G = len(D)
    S = symmetric(D)
    bound = (np.float32(2.0) * nu) * np.float32(tol)
    order = 1
    if all(S[g] <= bound for g in range(1, G)):
        order = 0
    else:
        for m in sorted(orders):
            if G % m == 0 and all(S[k * G // m] <= bound for k in range(1, m)):
                order = m
    width = max(orders) if width is None else width
    angles = np.zeros(width, np.float32)
    for k in range(order):
        angles[k] = np.float32(2 * np.pi * k / order)
    return order, order, angles


# ---- seeded families -------------------------------------------------------------------------------------------------------------
FAMILIES = {"wedge": 1, "box": 2, "square": 4, "triangle": 3, "cylinder": 0}   # name -> the order of its yaw symmetry (0: continuous)
HALF_HEIGHT = 0.3


def _canonical(name, N, g):
    u = torch.rand(N, 3, generator=g, dtype=torch.float64)
    y = (u[:, 1] * 2 - 1) * HALF_HEIGHT
    if name in ("wedge", "box", "square"):
        hx, hz = (0.8, 0.8) if name == "square" else (0.6, 1.0)
        x, z = (u[:, 0] * 2 - 1) * hx, (u[:, 2] * 2 - 1) * hz
        if name == "wedge":
            x = x * (0.4 + 0.6 * (z + 1.0) / 2.0)      # narrow at z = -1, full width at z = +1
    elif name == "triangle":                            # uniform in the equilateral triangle of circumradius 1
        r1, r2 = torch.sqrt(u[:, 0]), u[:, 2]
        w = torch.stack([1 - r1, r1 * (1 - r2), r1 * r2], 1)
        a = torch.tensor([math.pi / 2, math.pi / 2 + 2 * math.pi / 3, math.pi / 2 + 4 * math.pi / 3], dtype=torch.float64)
        x, z = w @ torch.cos(a), w @ torch.sin(a)
    elif name == "cylinder":
        r, a = 0.8 * torch.sqrt(u[:, 0]), 2 * math.pi * u[:, 2]
        x, z = r * torch.cos(a), r * torch.sin(a)
    else:
        raise KeyError(name)
    return torch.stack([x, y, z], 1)


def turned(xyz, theta):
    """float32 cloud turned about +Y by theta (float64 arithmetic, rounded once)."""
    p = np.asarray(xyz, np.float64)
    c, s = math.cos(theta), math.sin(theta)
    return np.stack([c * p[:, 0] + s * p[:, 2], p[:, 1], c * p[:, 2] - s * p[:, 0]], 1).astype(np.float32)


def family(name, N, seed):
    """(N, 3) float32: the family's shape filled uniformly, at a random yaw and a random offset."""
    g = torch.Generator().manual_seed(SEED + 1000 * sorted(FAMILIES).index(name) + seed)
    p = _canonical(name, N, g).numpy()
    theta = float(torch.rand(1, generator=g, dtype=torch.float64)) * 2 * math.pi
    offset = (torch.rand(3, generator=g, dtype=torch.float64).numpy() - 0.5)
    return (turned(p, theta).astype(np.float64) + offset).astype(np.float32)


def batch(names, N, seed):
    return np.stack([family(n, N, seed + i) for i, n in enumerate(names)])


def centroid(xyz):
    return np.asarray(xyz, np.float64).mean(0).astype(np.float32)


def lattice():
    """(32, 3) float32 integer lattice 4 x 2 x 4 (x, y, z) with its explicit centre: exactly 4-fold about it, full of exact ties."""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(2), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    return (g + np.array([3, 0, -5])).astype(np.float32), np.array([4.5, 0.0, -3.5], np.float32)


# ---- classification cases: N = 1024, G = 24 ----------------------------------------------------------------------------------------
CLASS_N, CLASS_G, CLASS_SEEDS = 1024, 24, (0, 1, 2)
ADMIT_TRUE, ADMIT_FALSE = 1.15, 1.5


def admitted(name, seed):
    """The seeded case and whether the float64 restatement admits it: every true-symmetry score <= 1.15 and, for every candidate order the
    family does not have, that order's worst score >= 1.5.  -> (xyz, admitted, worst true score, smallest false-order score)"""
    xyz = family(name, CLASS_N, seed)
    D, nu = profile(xyz, centroid(xyz), grid_table(CLASS_G), np.float64)
    score = symmetric(D) / (2.0 * nu)
    G, true_order = CLASS_G, FAMILIES[name]
    true_g = list(range(1, G)) if true_order == 0 else [k * G // true_order for k in range(1, true_order)]
    worst_true = max((score[g] for g in true_g), default=0.0)
    false_orders = [m for m in ORDERS if G % m == 0 and true_order != 0 and true_order % m != 0]
    least_false = min((max(score[k * G // m] for k in range(1, m)) for m in false_orders), default=math.inf)
    return xyz, worst_true <= ADMIT_TRUE and least_false >= ADMIT_FALSE, worst_true, least_false


# ---- parity cases ------------------------------------------------------------------------------------------------------------------
PARITY_N = (1, 2, 63, 64, 65, 255, 256, 257)
PARITY_G = (1, 2, ANGLE_BLOCK - 1, ANGLE_BLOCK, ANGLE_BLOCK + 1, 9, 2 * ANGLE_BLOCK - 1)
PARITY_G = tuple(sorted(set(PARITY_G)))
PARITY_B = (1, 3)
TILE_N = (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
NAMES = ("wedge", "box", "square", "triangle", "cylinder")


def parity_cloud(B, N, seed=0):
    """(B, N, 3) float32: the families in turn."""
    return batch([NAMES[(seed + b) % len(NAMES)] for b in range(B)], N, 100 + seed)
