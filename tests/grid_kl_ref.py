"""The mixture KL on the decode grid (pnpp_mvm_grid_kl) restated in numpy float64, with its three analytic gradients, the multi-peak
head and its backward in float64, and the seeded case table of tests/test_gpu_grid_kl.py.  Written sample by sample, for reading; the
exponentially scaled Bessel functions are torch.special.i0e / i1e in float64.

    q(t) = sum_{j < K_gt} v_j vM(t; nu_j, lambda_j)     v normalised by the sum of its positive entries, entries <= 0 skipped
    p(t) = sum_i w_i vM(t; mu_i, kappa_i)               all components, weights as given, weights <= 0 skipped
    loss = (2 pi / G) sum_g q(t_g) (log q(t_g) - log p(t_g)),   t_g = 2 pi g / G,  G = num - 1
"""
import math

import numpy as np
import torch

TWO_PI = 2.0 * math.pi
KAPPA_CLAMP = 500.0


def _i0e(k):
    return torch.special.i0e(torch.as_tensor(np.asarray(k, dtype=np.float64))).numpy()


def _i1e(k):
    return torch.special.i1e(torch.as_tensor(np.asarray(k, dtype=np.float64))).numpy()


def _lse(a):   # over axis 0
    m = a.max(axis=0)
    return m + np.log(np.exp(a - m).sum(axis=0))


def sample(mu, kappa, weight, gt, k_gt, num=360):
    """One sample.  mu, kappa, weight (K,), gt (K, 3) rows (nu, lambda, v), k_gt int -> loss, dmu (K,), dkappa (K,), dweight (K,)."""
    mu, kappa, weight, gt = (np.asarray(a, dtype=np.float64) for a in (mu, kappa, weight, gt))
    K, G = mu.shape[0], int(num) - 1
    nothing = (0.0, np.zeros(K), np.zeros(K), np.zeros(K))
    kg = min(max(int(k_gt), 0), K)
    v = gt[:kg, 2]
    used = v > 0.0
    if kg == 0 or not v[used].sum() > 0.0:
        return nothing
    th = np.arange(G, dtype=np.float64) * TWO_PI / G
    nu, lam, v = gt[:kg, 0][used], np.clip(gt[:kg, 1][used], 0.0, KAPPA_CLAMP), v[used]
    lv = np.log(v / v.sum()) - np.log(TWO_PI * _i0e(lam))
    lq = _lse(lam[:, None] * (np.cos(th[None, :] - nu[:, None]) - 1.0) + lv[:, None])

    kc = np.clip(kappa, 0.0, KAPPA_CLAMP)
    passes = ((kappa >= 0.0) & (kappa <= KAPPA_CLAMP)).astype(np.float64)
    i0 = _i0e(kc)
    A = _i1e(kc) / i0
    c, s = np.cos(th[None, :] - mu[:, None]), np.sin(th[None, :] - mu[:, None])
    e = kc[:, None] * (c - 1.0) - np.log(TWO_PI * i0)[:, None]          # log vM_i on the grid
    live = weight > 0.0
    lp = _lse(e[live] + np.log(weight[live])[:, None])
    cst = TWO_PI / G
    loss = cst * np.sum(np.exp(lq) * (lq - lp))
    qv = np.exp(lq[None, :] + e - lp[None, :])                           # q vM_i / p
    qr = np.where(live, weight, 0.0)[:, None] * qv                       # q r_i
    return (loss, -cst * kc * (qr * s).sum(axis=1), -cst * (qr * (c - A[:, None])).sum(axis=1) * passes, -cst * qv.sum(axis=1))


def batch(mu, kappa, weight, vm_gt, K_gt, num=360):
    """(B,K) x 3, (B,K,3), (B,) -> loss (B,), dmu, dkappa, dweight (B,K), float64."""
    rows = [sample(mu[b], kappa[b], weight[b], vm_gt[b], K_gt[b], num) for b in range(len(mu))]
    return tuple(np.stack([np.asarray(r[i], dtype=np.float64) for r in rows]) for i in range(4))


# ---- the head (models/pointnet_pp_mvM.py) and its backward, float64 throughout -------------------------------------------------------
def head(pi_raw, mu_raw, kappa_raw, temp, kappa_max):
    """One sample: pi_raw (K,), mu_raw (2K,), kappa_raw (K,) -> mu, kappa, weight (K,)."""
    pi_raw, mu_raw, kappa_raw = (np.asarray(a, dtype=np.float64) for a in (pi_raw, mu_raw, kappa_raw))
    z = pi_raw / temp
    w = np.exp(z - z.max())
    w /= w.sum()
    r = mu_raw.reshape(-1, 2)
    u = r / np.maximum(np.hypot(r[:, 0], r[:, 1]), 1e-4)[:, None]
    dead = np.hypot(u[:, 0], u[:, 1]) < 1e-3
    mu = np.where(dead, 0.0, np.arctan2(u[:, 1], u[:, 0]))
    sp = np.where(kappa_raw > 20.0, kappa_raw, np.log1p(np.exp(np.minimum(kappa_raw, 20.0)))) + 1e-6
    return mu, np.minimum(sp, kappa_max), w


def head_bwd(pi_raw, mu_raw, kappa_raw, temp, kappa_max, dmu, dkappa, dweight):
    """The gradient of a scalar with respect to the raw head outputs from its gradient with respect to (mu, kappa, weight)."""
    pi_raw, mu_raw, kappa_raw = (np.asarray(a, dtype=np.float64) for a in (pi_raw, mu_raw, kappa_raw))
    _, _, w = head(pi_raw, mu_raw, kappa_raw, temp, kappa_max)
    dpi = w * (dweight - np.dot(w, dweight)) / temp
    r = mu_raw.reshape(-1, 2)
    dmr = np.zeros_like(r)
    for k in range(r.shape[0]):
        n = math.hypot(r[k, 0], r[k, 1])
        c, s = r[k] / max(n, 1e-4)
        n2 = c * c + s * s
        if math.sqrt(n2) < 1e-3:
            continue                                   # the fallback mu = 0 is a constant
        dc, ds = -s / n2 * dmu[k], c / n2 * dmu[k]
        if n >= 1e-4:
            proj = dc * c + ds * s
            dmr[k] = (dc - c * proj) / n, (ds - s * proj) / n
        else:
            dmr[k] = dc / 1e-4, ds / 1e-4
    sp = np.where(kappa_raw > 20.0, kappa_raw, np.log1p(np.exp(np.minimum(kappa_raw, 20.0)))) + 1e-6
    sig = np.where(kappa_raw > 20.0, 1.0, 1.0 / (1.0 + np.exp(-kappa_raw)))
    return dpi, dmr.reshape(-1), np.where(sp <= kappa_max, dkappa * sig, 0.0)


def descent(steps=40, lr=0.1, max_K=4, temp=0.7, kappa_max=80.0, num=360):
    """Plain gradient descent on the raw head parameters of one sample, the descent case of the GPU test: the losses before each step."""
    pi_raw, kappa_raw = np.zeros(max_K), np.zeros(max_K)
    mu_raw = descent_mu_raw(max_K).astype(np.float64)
    gt, losses = descent_gt(max_K).astype(np.float64), []
    for _ in range(steps + 1):
        mu, kap, w = head(pi_raw, mu_raw, kappa_raw, temp, kappa_max)
        loss, dmu, dk, dw = sample(mu, kap, w, gt, 2, num)
        losses.append(float(loss))
        dpi, dmr, dkr = head_bwd(pi_raw, mu_raw, kappa_raw, temp, kappa_max, dmu, dk, dw)
        pi_raw, mu_raw, kappa_raw = pi_raw - lr * dpi, mu_raw - lr * dmr, kappa_raw - lr * dkr
    return losses


def descent_mu_raw(max_K=4):
    ang = TWO_PI * np.arange(max_K) / max_K - math.pi + 0.1
    return np.stack((np.cos(ang), np.sin(ang)), axis=1).reshape(-1).astype(np.float32)


def descent_gt(max_K=4):
    gt = np.zeros((max_K, 3), np.float32)
    gt[0], gt[1] = (0.3, 8.0, 0.5), (0.3 - math.pi, 8.0, 0.5)
    return gt


# ---- the loophole row of match_loss: the prediction copies two ground-truth peaks but carries 0.9 of its weight elsewhere ------------
def loophole_row():
    gt = np.zeros((4, 3))
    gt[0], gt[1] = (0.5, 8.0, 0.5), (0.5 - math.pi, 8.0, 0.5)
    mu = np.array([0.5, 0.5 - math.pi, 2.0, -1.0])
    kappa = np.array([8.0, 8.0, 1e-6, 1e-6])
    weight = np.array([0.05, 0.05, 0.45, 0.45])
    return mu, kappa, weight, gt, 2


# ---- the case table of the GPU parity test ------------------------------------------------------------------------------------------
KAPPAS = np.array([1e-6, 8.0, 80.0, 500.0, 600.0], np.float32)
BROAD = np.array([1e-6, 0.5, 2.0, 8.0], np.float32)
MAX_KS, GRIDS = (1, 2, 3, 4, 8), (2, 8, 255, 256, 257, 359, 1024)
PI32 = np.float32(math.pi)


def rows(B, K, seed):
    """B rows at max_K = K: K_gt cycles through 0 .. K + 1; ground-truth weights that do not sum to 1, with exact zeros; predicted
    weights with exact zeros; coincident components; mu at +-pi; kappa from KAPPAS on both sides.  A row with a zero predicted weight
    keeps component 0 live and broad: d loss / d w_i of a weightless sharp component where p underflows is beyond float32 (and float64).
    """
    rng = np.random.RandomState(seed)
    mu = rng.uniform(-math.pi, math.pi, (B, K)).astype(np.float32)
    kappa = KAPPAS[rng.randint(0, len(KAPPAS), (B, K))]
    some = rng.rand(B, K) < 0.3                            # and off the table
    kappa[some] = rng.uniform(0.1, 30.0, (B, K)).astype(np.float32)[some]
    weight = rng.uniform(0.05, 1.0, (B, K)).astype(np.float32)
    weight /= weight.sum(axis=1, keepdims=True)           # as a softmax gives them; not renormalised by the loss in any case
    gt = np.zeros((B, K, 3), np.float32)
    gt[:, :, 0] = rng.uniform(-math.pi, math.pi, (B, K))
    gt[:, :, 1] = KAPPAS[rng.randint(0, len(KAPPAS), (B, K))]
    gt[:, :, 2] = rng.uniform(0.1, 2.0, (B, K))
    k_gt = (np.arange(B) % (K + 2)).astype(np.int32)
    k_gt[0] = K                                            # a batch of one is a full row
    for b in range(B):
        kind = (b // (K + 2)) % 5
        if kind == 1 and K >= 2:                           # exact zeros among the predicted weights
            weight[b, 1 + rng.randint(0, K - 1)] = 0.0
            kappa[b, 0] = BROAD[rng.randint(0, len(BROAD))]
        elif kind == 2 and K >= 2:                         # coincident components, on both sides
            mu[b, 1], kappa[b, 1] = mu[b, 0], kappa[b, 0]
            gt[b, 1, :2] = gt[b, 0, :2]
        elif kind == 3:                                    # mu at +-pi
            mu[b, 0], gt[b, 0, 0] = PI32, -PI32
            if K >= 2:
                mu[b, 1] = -PI32
        elif kind == 4 and K >= 2:                         # a ground-truth weight of exactly 0
            gt[b, rng.randint(0, K), 2] = 0.0
    return mu, kappa, weight, gt, k_gt


def kappa_rows():
    """max_K = 1, one row per (kappa, lambda) of KAPPAS x KAPPAS: every clamp edge on both sides with nothing else in the way."""
    n = len(KAPPAS)
    mu = np.full((n * n, 1), 0.4, np.float32)
    kappa = np.repeat(KAPPAS, n)[:, None].copy()
    weight = np.ones((n * n, 1), np.float32)
    gt = np.zeros((n * n, 1, 3), np.float32)
    gt[:, 0, 0], gt[:, 0, 1], gt[:, 0, 2] = 0.1, np.tile(KAPPAS, n), 1.0
    return mu, kappa, weight, gt, np.ones(n * n, np.int32)


def cases():
    """name -> (mu, kappa, weight, vm_gt, K_gt, num): B = 65 at every (max_K, grid) pair, B = 1 and 3 at two, and the kappa table."""
    out = {}
    for K in MAX_KS:
        for G in GRIDS:
            out[f"B65-K{K}-G{G}"] = (*rows(65, K, 1000 * K + G), G + 1)
    for B in (1, 3):
        out[f"B{B}-K4-G359"] = (*rows(B, 4, 77 + B), 360)
        out[f"B{B}-K8-G257"] = (*rows(B, 8, 99 + B), 258)
    out["kappa-table"] = (*kappa_rows(), 360)
    return out
