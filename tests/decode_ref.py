"""Float64 restatement of pnpp_mvm_decode and pnpp_orient_eval (include/pnpp_hip.h) in numpy: what the device kernels are compared
with.  Written sample by sample, for reading; the exponentially scaled Bessel function is torch.special.i0e in float64."""
import math

import numpy as np
import torch

TWO_PI = 2.0 * math.pi
ROUNDS, POINTS = 8, 65
BINS, STRIDE = 360, 728


def _i0e(k):
    return torch.special.i0e(torch.as_tensor(np.asarray(k, dtype=np.float64))).numpy()


class Mixture:
    """One sample's p(x) = sum_k w_k exp(kappa_k (cos(x - mu_k) - 1)) / (2 pi i0e(kappa_k)), unnormalised, float64."""

    def __init__(self, mu, kappa, weight, count):
        self.mu = np.asarray(mu, np.float64)[:count]
        kap = np.asarray(kappa, np.float64)[:count]
        self.kappa = np.where(kap > 0.0, kap, 0.0)
        w = np.ones(count) if weight is None else np.asarray(weight, np.float64)[:count]
        self.coef = w / (TWO_PI * _i0e(self.kappa)) if count else w

    def __call__(self, x):
        x = np.asarray(x, np.float64)
        p = np.zeros(x.shape)
        for m, k, c in zip(self.mu, self.kappa, self.coef):
            p = p + c * np.exp(k * (np.cos(x - m) - 1.0))
        return p


def grid(num):
    G = num - 1
    return np.arange(G, dtype=np.float64) * TWO_PI / G


def density(mu, kappa, weight=None, counts=None, num=360):
    """(B, G) float64: p / (sum p + 1e-8)."""
    B, K = np.shape(mu)
    th = grid(num)
    out = np.zeros((B, th.size))
    for b in range(B):
        p = Mixture(mu[b], kappa[b], None if weight is None else weight[b], _count(counts, b, K))(th)
        out[b] = p / (p.sum() + 1e-8)
    return out


def _count(counts, b, K):
    return K if counts is None else int(min(max(int(counts[b]), 0), K))


def _section(p, lo, hi):
    """Value sectioning: 65 equispaced points, the two sub-cells around the (first, interior-clamped) arg-max, 8 rounds."""
    for _ in range(ROUNDS):
        x = lo + np.arange(POINTS) * ((hi - lo) / (POINTS - 1))
        j = int(min(max(int(np.argmax(p(x))), 1), POINTS - 2))
        lo, hi = x[j - 1], x[j + 1]
    mid = 0.5 * (lo + hi)
    return mid, float(p(mid))


def decode(mu, kappa, weight=None, counts=None, num=360, rel_height=0.1):
    """-> dict(modes (B,K), heights (B,K), n_modes (B,), angle (B,), near_tie (B,) bool) in float64.
    near_tie: two candidate heights within 1e-9 relative, or a height within 1e-6 relative of the rel_height cut -- the order or the
    count of such a sample's modes is not decided at float64."""
    mu, kappa = np.asarray(mu, np.float64), np.asarray(kappa, np.float64)
    B, K = mu.shape
    G = num - 1
    th = grid(num)
    step = TWO_PI / G
    modes, heights = np.full((B, K), np.nan), np.zeros((B, K))
    n_modes, near = np.zeros(B, np.int32), np.zeros(B, bool)
    rel = float(np.float32(rel_height))
    for b in range(B):
        p = Mixture(mu[b], kappa[b], None if weight is None else weight[b], _count(counts, b, K))
        g = p(th)
        cand = [i for i in range(G) if g[i] > g[i - 1] and g[i] >= g[(i + 1) % G]]
        found = []
        for i in cand:
            x, h = _section(p, th[i] - step, th[i] + step)
            x = x + TWO_PI if x < 0.0 else x
            x = x - TWO_PI if x >= TWO_PI else x
            found.append((h, x))
        found.sort(key=lambda t: (-t[0], t[1]))
        hs = [h for h, _ in found]
        for a, c in zip(hs, hs[1:]):
            near[b] |= abs(a - c) <= 1e-9 * max(a, c)
        kept = [(h, x) for h, x in found if h >= rel * found[0][0]][:K]
        if found:
            cut = rel * found[0][0]
            near[b] |= any(abs(h - cut) <= 1e-6 * max(cut, 1e-300) for h in hs[1:])
        n_modes[b] = len(kept)
        for s, (h, x) in enumerate(kept):
            modes[b, s] = x - TWO_PI if x > math.pi else x
            heights[b, s] = h
    return {"modes": modes, "heights": heights, "n_modes": n_modes, "angle": modes[:, 0].copy(), "near_tie": near}


def wrap_abs(d):
    d = np.asarray(d, np.float64)
    return np.abs(d - TWO_PI * np.rint(d / TWO_PI))


def orient_eval(modes, n_modes, angle, mu_gt=None, kappa_gt=None, vm_gt=None, K_gt=None, labels=None, n_labels=1):
    """-> dict(top1, cover (B,) degrees float64, -1 when excluded; count_ok (B,) int; acc (n_labels * STRIDE + 1,) uint64 as the
    kernel lays it out; edge (B,) float64: the distance in degrees of the sample's errors from the nearest histogram bin edge)."""
    modes = np.asarray(modes, np.float64)
    B, K = modes.shape
    if vm_gt is None:
        vm_gt = np.stack([np.asarray(mu_gt, np.float64), np.asarray(kappa_gt, np.float64)], -1)[:, None, :]
        K_gt = np.ones(B, np.int64)
    vm_gt = np.asarray(vm_gt, np.float64)
    Kmax = vm_gt.shape[1]
    top1, cover, ok = np.full(B, -1.0), np.full(B, -1.0), np.zeros(B, np.int32)
    edge = np.full(B, np.inf)
    acc = np.zeros(n_labels * STRIDE + 1, np.uint64)
    for b in range(B):
        nm = int(min(max(int(n_modes[b]), 0), K))
        kg = int(min(max(int(K_gt[b]), 0), Kmax))
        ok[b] = int(nm == int(K_gt[b]))
        A = acc[(0 if labels is None else int(min(max(int(labels[b]), 0), n_labels - 1))) * STRIDE:]
        incl = kg > 0 and bool((vm_gt[b, :kg, 1] > 1e-6).any()) and nm > 0
        if incl:
            gt = vm_gt[b, :kg, 0]
            top1[b] = np.degrees(wrap_abs(float(angle[b]) - gt).min())
            cover[b] = np.degrees(max(wrap_abs(modes[b, :nm] - m).min() for m in gt))
            for e, off in ((top1[b], 0), (cover[b], BINS)):
                A[off + min(int(e * 2.0), BINS - 1)] += np.uint64(1)
                edge[b] = min(edge[b], abs(e * 2.0 - round(e * 2.0)) / 2.0 if e < 179.75 else np.inf)
            A[2 * BINS] += np.uint64(1)
            A[2 * BINS + 3] += np.uint64(int(np.rint(top1[b] * 1e6)))
            A[2 * BINS + 4] += np.uint64(int(np.rint(cover[b] * 1e6)))
        else:
            A[2 * BINS + 1] += np.uint64(1)
        if ok[b]:
            A[2 * BINS + 2] += np.uint64(1)
    acc[-1] = np.uint64(B)
    return {"top1": top1, "cover": cover, "count_ok": ok, "acc": acc, "edge": edge}


# ---- the seeded inputs of the decode tests -------------------------------------------------------------------------------------
SHAPES = [(B, K, num) for B in (1, 33) for K in (1, 4, 8) for num in (9, 65, 360, 1025)]
NEAR_TIE_CAP = 0.02   # the share of samples a test may leave out because float64 itself does not decide them


def random_case(B, K, seed):
    """mu uniform on the circle, kappa log-uniform on [0.5, 80], Dirichlet weights; float32, as the device receives them."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-math.pi, math.pi, (B, K)).astype(np.float32)
    kappa = np.exp(rng.uniform(math.log(0.5), math.log(80.0), (B, K))).astype(np.float32)
    weight = rng.dirichlet(np.ones(K), B).astype(np.float32)
    return mu, kappa, weight


def case_seed(B, K, num):
    return 1000 * B + 10 * K + num
