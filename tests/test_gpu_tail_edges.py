"""The tail of every training step -- output heads, von-Mises KL losses, matching, the fused tail launches with the riding
centre draw, the flat-buffer Adam and its clip -- steered at the branches of csrc/loss_kernels.hip, step_tail_kernels.hip and optim_kernels.hip on purpose, against references
that share nothing with the kernels: tests/golden/tail_edges.npz (mpmath, oracle/make_tail_golden.py; pinned on the CPU by
tests/test_tail_golden_cpu.py), float64 autograd of the oracle's expressions, and float64 numpy restatements of torch.optim.Adam.

Gates are the ones the suite already uses (G5 = 1e-5 * max(1, |ref|) for heads and losses, the gates of
tests/test_gpu_head_loss.py for the fused tails) or are derived where they are set (Adam).  Every test prints the worst error it saw
as `worst[<family>]`, so the room under each gate is on record in the log."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

G5 = 1e-5
U = 2.0 ** -24                      # one float32 rounding, relative


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _n(t):
    return t.detach().cpu().double().numpy()


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _g5(got, ref):
    """Worst |got - ref| / max(1, |ref|); the caller asserts <= G5 (or the 2e-5 of test_mvm_head_forward_backward)."""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


def _report(family, **errs):
    print("  worst[" + family + "] " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))


@pytest.fixture(scope="module")
def ops():
    from pnpp_hip import ops
    return ops


@pytest.fixture(scope="module")
def L():
    from pnpp_hip import _lib
    return _lib


@pytest.fixture(scope="module")
def edges(golden):
    g = golden("tail_edges.npz")
    return {k: g[k] for k in g.files}


class _Calls:
    """Counts the calls of one C entry point (which of an op's two routes ran) while passing them through."""

    def __init__(self, monkeypatch, L, name):
        self.n = 0
        real = getattr(L.lib(), name)

        def through(*a):
            self.n += 1
            return real(*a)
        monkeypatch.setattr(L.lib(), name, through, raising=False)


# ------------------------------------------------------------------------------------------------------------------------
# single-peak KL
# ------------------------------------------------------------------------------------------------------------------------
def test_kl_single_whole_sweep(ops, edges):
    """ops.kl_von_mises_single on the full grid: both Chebyshev tables of i0e / i1e and their switch at 8, the kappa_p <= 1e-6
    branch from either side, kappa past the float32 overflow of I0 (89) up to 1e6, where A' = 1 - A^2 - A/k cancels."""
    c = _t(edges["inputs"]).cuda()
    mu = c[:, 0].clone().requires_grad_(True)
    kap = c[:, 1].clone().requires_grad_(True)
    v = ops.kl_von_mises_single(mu, kap, c[:, 2].contiguous(), c[:, 3].contiguous())
    v.sum().backward()
    ref = edges["single"]
    e = [_g5(_n(v), ref[:, 0]), _g5(_n(mu.grad), ref[:, 1]), _g5(_n(kap.grad), ref[:, 2])]
    _report("single KL", value=e[0], dmu=e[1], dkappa=e[2])
    assert max(e) <= G5


def _inverse_softplus(kappa32):
    """float32 o1 whose softplus is (as near as float32 allows) the given kappa: o1 = kappa above the threshold 20, else the
    float64 inverse log(expm1(kappa)); of its float32 neighbours the one whose softplus rounds back to kappa is taken where one
    does (below ~1e-3 none can: softplus is flatter there than float32 is fine).  kappa = 0 is exp(-200) = 1e-87, 0 in float32."""
    out = np.empty_like(kappa32)
    for i, k in enumerate(kappa32.astype(np.float64)):
        if k > 20.0:
            out[i] = k
        elif k == 0.0:
            out[i] = -200.0
        else:
            o = np.float32(math.log(math.expm1(k)))
            cand = [o]
            for _ in range(3):
                cand = [np.nextafter(cand[0], np.float32(-np.inf))] + cand + [np.nextafter(cand[-1], np.float32(np.inf))]
            hit = [x for x in cand if np.float32(math.log1p(math.exp(float(x)))) == np.float32(k)]
            out[i] = min(hit, key=lambda x: abs(float(x) - float(o))) if hit else o
    return out


def test_kl_single_four_routes(ops, edges):
    """The sweep's rows through the head routes: vm_head_kl_fused, vm_head_kl_loss (none / mean; 595 rows: the B > 256 strided loop
    and ten 64-sample chunks of vm_head_kl_chunk) and vm_fc_head_kl_loss_backward (K = 2, fc3 = identity, so o = x exactly).
    mu_p = tanh(0) pi = 0 and mu_q = -(mu_p - mu_q) of the row; o1 is the inverse softplus of the row's kappa_p.  Routes agree as
    tests/test_gpu_head_loss.py requires (bit-equal where they share device functions, else rtol 1e-6); rows whose kappa came out
    of the head as exactly the swept float32 are held against the fixture too."""
    inp, ref = edges["inputs"], edges["single"]
    B = len(inp)
    o_np = np.stack([np.zeros(B, np.float32), _inverse_softplus(inp[:, 1])], 1)
    o = _t(o_np).cuda()
    mu_gt, kap_gt = _t(-(inp[:, 0] - inp[:, 2])).cuda(), _t(inp[:, 3].copy()).cuda()
    # route 1: one launch, no autograd
    mu, kap, lv, d_o = ops.vm_head_kl_fused(o, mu_gt, kap_gt)
    assert torch.equal(mu, torch.zeros_like(mu))
    # route 0: head op + KL op through autograd
    og = o.clone().requires_grad_(True)
    mu0, kap0 = ops.vm_head(og)
    lv0 = ops.kl_von_mises_single(mu0, kap0, mu_gt, kap_gt)
    lv0.sum().backward()
    assert torch.equal(mu0, mu) and torch.equal(kap0, kap) and torch.equal(lv0.detach(), lv)
    assert torch.allclose(d_o, og.grad, rtol=1e-6, atol=1e-7)
    # route 2: the autograd op, per sample (the same kernel) and mean (vm_head_kl_chunk: the same float64 operations)
    o2 = o.clone().requires_grad_(True)
    lv2 = ops.vm_head_kl_loss(o2, mu_gt, kap_gt, reduction="none")
    lv2.sum().backward()
    assert torch.equal(lv2.detach(), lv) and torch.equal(o2.grad, d_o)
    o3 = o.clone().requires_grad_(True)
    lm = ops.vm_head_kl_loss(o3, mu_gt, kap_gt, reduction="mean")
    lm.backward()
    mean64 = float(lv.double().mean())
    assert abs(float(lm) - mean64) <= 1e-6 * abs(mean64)
    assert torch.allclose(o3.grad, d_o / B, rtol=1e-6, atol=1e-7 / B)
    # route 3: fc3 + head + KL + mean + backward in one launch; W = I, b = 0: o = x and dx = d_o to the bit
    lin = nn.Linear(2, 2).cuda()
    with torch.no_grad():
        lin.weight.copy_(torch.eye(2))
        lin.bias.zero_()
    x = o.clone().requires_grad_(True)
    lf = ops.vm_fc_head_kl_loss_backward(x, lin, mu_gt, kap_gt)
    assert torch.equal(lf, lm.detach()) and torch.equal(x.grad, o3.grad)
    d64, x64 = _n(o3.grad), o_np.astype(np.float64)
    assert _rel(_n(lin.weight.grad), d64.T @ x64) < 2e-5 and _rel(_n(lin.bias.grad), d64.sum(0)) < 2e-5
    # against the fixture, where the head's float32 kappa is the swept one
    landed = _n(kap) == inp[:, 1].astype(np.float64)
    must = (inp[:, 1] > 20.0) | (inp[:, 1] == 0.0)
    assert landed[must].all() and must.sum() == 8 * 35
    sig = np.where(o_np[:, 1] > 20.0, 1.0, 1.0 / (1.0 + np.exp(-o_np[:, 1].astype(np.float64))))
    e = [_g5(_n(lv)[landed], ref[landed, 0]), _g5(_n(d_o)[landed, 0], ref[landed, 1] * math.pi),
         _g5(_n(d_o)[landed, 1], ref[landed, 2] * sig[landed])]
    _report("single KL, head routes", rows=float(landed.sum()), value=e[0], d_o0=e[1], d_o1=e[2])
    assert max(e) <= G5


# ------------------------------------------------------------------------------------------------------------------------
# vm head
# ------------------------------------------------------------------------------------------------------------------------
def test_vm_head_thresholds_and_saturation(ops):
    """mu = tanh(o0) pi, kappa = softplus(o1) with o1 on and one float32 either side of the softplus threshold 20, far below it
    (kappa ~ e^-100, a float32 denormal) and far above; o0 from 0 to saturation.  Saturated tanh gives exactly zero d_o[:, 0]."""
    f = np.float32
    o1s = [-100.0, -20.0, 0.0, np.nextafter(f(20), f(0)), 20.0, np.nextafter(f(20), f(30)), 88.0, 1e4]
    o0s = [0.0, 1e-4, -1e-4, 9.0, -9.0, 20.0, -20.0, 1e4, -1e4]
    o = torch.tensor(list(itertools.product(o0s, o1s)), dtype=torch.float32)
    g = torch.Generator().manual_seed(11)
    gm, gk = torch.randn(len(o), generator=g), torch.randn(len(o), generator=g)
    od = o.double().requires_grad_(True)
    mu_ref, kap_ref = torch.tanh(od[:, 0]) * math.pi, torch.nn.functional.softplus(od[:, 1])
    (mu_ref * gm.double() + kap_ref * gk.double()).sum().backward()
    og = o.clone().cuda().requires_grad_(True)
    mu, kap = ops.vm_head(og)
    (mu * gm.cuda() + kap * gk.cuda()).sum().backward()
    tiny = float(np.finfo(np.float32).tiny)      # below it float32 has no 1e-6 to give
    for got, r in ((mu, mu_ref), (kap, kap_ref)):
        assert np.all(np.abs(_n(got) - _n(r)) <= 1e-6 * np.abs(_n(r)) + tiny)
    e = _g5(_n(og.grad), _n(od.grad))
    _report("vm head", mu=_rel(_n(mu), _n(mu_ref)), kappa=_rel(_n(kap), _n(kap_ref)), d_o=e)
    assert e <= G5
    sat = (o[:, 0].abs() >= 20.0).cuda()
    assert int(sat.sum()) == 4 * len(o1s)
    assert torch.all(og.grad[sat, 0] == 0) and torch.all(og.grad[~sat, 0] != 0)
    # the one-launch head + KL takes the same branches
    mu2, kap2, _, d_o = ops.vm_head_kl_fused(og.detach(), torch.full_like(mu, 0.3), torch.full_like(mu, 8.0))
    assert torch.equal(mu2, mu.detach()) and torch.equal(kap2, kap.detach()) and torch.all(d_o[sat, 0] == 0)


# ------------------------------------------------------------------------------------------------------------------------
# multi-peak KL through match_loss at max_K = 1
# ------------------------------------------------------------------------------------------------------------------------
def test_kl_multi_whole_sweep_through_match_loss(ops, edges):
    """max_K = K = 1: loss = w c / (w + 1e-8) with c the multi-peak KL of the row -- clamps at 1e-6 and 500 from either side with
    the gated d/d kappa, the wrapped angle at +-float32(pi) and 2 pi."""
    inp, ref = edges["inputs"], edges["multi"]
    B = len(inp)
    w_np = np.random.default_rng(5).uniform(0.1, 1.0, B).astype(np.float32)
    mu, kap, w = (_t(a.reshape(B, 1).copy()).cuda().requires_grad_(True) for a in (inp[:, 0], inp[:, 1], w_np))
    vm = torch.zeros(B, 1, 3)
    vm[:, 0, 0], vm[:, 0, 1], vm[:, 0, 2] = _t(inp[:, 2].copy()), _t(inp[:, 3].copy()), 1.0
    lv = ops.match_loss(mu, kap, w, vm.cuda(), torch.ones(B, dtype=torch.int64).cuda())
    lv.sum().backward()
    w64 = w_np.astype(np.float64)
    S = w64 + 1e-8
    e = [_g5(_n(lv), w64 * ref[:, 0] / S), _g5(_n(mu.grad), w64 / S * ref[:, 1]), _g5(_n(kap.grad), w64 / S * ref[:, 2]),
         _g5(_n(w.grad), ref[:, 0] * 1e-8 / (S * S))]
    _report("multi KL", loss=e[0], dmu=e[1], dkappa=e[2], dw=e[3])
    assert max(e) <= G5
    assert torch.all(kap.grad[(kap < 1e-6) | (kap > 500.0)] == 0)


def test_kl_multi_non_finite_inputs(ops, oracle):
    """mu = +-inf / NaN and kappa = NaN make the cost NaN: nan_to_num turns it into the constant 1e6, which has no gradient;
    kappa = +inf is clamped to 500 (finite cost, gradient for mu, none for kappa).  Loss and d/dw are the float64 oracle's.  (For
    d/d mu, d/d kappa of the 1e6 rows autograd itself returns 0 * NaN = NaN: nan_to_num has zeroed the incoming gradient and the
    chain rule multiplies it with the NaN local derivative.  Zero is what the constant's gradient is.)"""
    inf, nan = float("inf"), float("nan")
    mu_v = [inf, -inf, nan, 0.5, 0.5, 0.5]
    kap_v = [2.0, 2.0, 2.0, inf, nan, 3.0]
    B = len(mu_v)
    col = lambda v: torch.tensor(v, dtype=torch.float32).reshape(B, 1)
    vm = torch.zeros(B, 1, 3)
    vm[:, 0, 0], vm[:, 0, 1], vm[:, 0, 2] = 0.2, 8.0, 1.0
    K = torch.ones(B, dtype=torch.int64)
    md, kd, wd = (t.double().requires_grad_(True) for t in (col(mu_v), col(kap_v), torch.full((B, 1), 0.7)))
    l64 = oracle.match_loss(md, kd, wd, vm.double(), K)
    l64.sum().backward()
    bad = np.array([True, True, True, False, True, False])
    assert np.all(_n(l64)[bad] > 0.99e6) and np.all(np.isfinite(_n(l64)))
    mu, kap, w = (t.detach().float().cuda().requires_grad_(True) for t in (md, kd, wd))
    lv = ops.match_loss(mu, kap, w, vm.cuda(), K.cuda())
    lv.sum().backward()
    print("  non-finite rows: loss", _n(lv), "dmu", _n(mu.grad).ravel(), "dkappa", _n(kap.grad).ravel())
    e = [_g5(_n(lv), _n(l64)), _g5(_n(w.grad), _n(wd.grad))]
    assert max(e) <= G5
    assert np.all(_n(mu.grad).ravel()[bad] == 0) and np.all(_n(kap.grad).ravel()[bad] == 0)
    ok = ~bad
    assert _g5(_n(mu.grad).ravel()[ok], _n(md.grad).ravel()[ok]) <= G5 and _g5(_n(kap.grad).ravel()[ok], _n(kd.grad).ravel()[ok]) <= G5
    assert float(kap.grad[3]) == 0.0 and float(mu.grad[3]) != 0.0            # +inf: clamped, its gate shut


# ------------------------------------------------------------------------------------------------------------------------
# matching
# ------------------------------------------------------------------------------------------------------------------------
MATCH_MAXK = (1, 2, 3, 5, 8)


def match_sizes(maxK):
    spb = 256 // (maxK * maxK)      # samples per workgroup of vm_match_loss_kernel
    return sorted({1, spb - 1, spb, spb + 1, 3 * spb + 2} - {0})


def match_case(maxK, B):
    """Continuous, seeded inputs; K_gt walks through max_K, 0 .. max_K - 1 and max_K + 3 (which the kernel and slicing both clamp)."""
    g = torch.Generator().manual_seed(1000 * maxK + B)
    mu = (torch.rand(B, maxK, generator=g) * 2 - 1) * math.pi
    kap = torch.rand(B, maxK, generator=g) * 30 + 0.05
    w = torch.softmax(torch.randn(B, maxK, generator=g), -1)
    vm = torch.zeros(B, maxK, 3)
    vm[..., 0] = (torch.rand(B, maxK, generator=g) * 2 - 1) * math.pi
    vm[..., 1] = torch.rand(B, maxK, generator=g) * 20 + 0.5
    vm[..., 2] = 1.0 / maxK
    vals = [maxK] + list(range(maxK)) + [maxK + 3]
    K = torch.tensor([vals[b % len(vals)] for b in range(B)])
    return mu, kap, w, vm, K


_perms = {}


def ambiguous(oracle, mu, kap, vm, K, gap=1e-4):
    """Per sample: do the best and the second-best distinct total of the float64 cost table, over every permutation, lie closer
    than `gap`?  There the float32-rounded table of the kernel may legitimately pick the other one."""
    B, maxK = mu.shape
    out = np.zeros(B, bool)
    for b in range(B):
        k = min(int(K[b]), maxK)
        if k < 2:
            continue
        cost = oracle.kl_multi(mu[b, :k, None].double(), kap[b, :k, None].double(), vm[b, None, :k, 0].double(),
                               vm[b, None, :k, 1].double()).numpy()
        if k not in _perms:
            _perms[k] = np.array(list(itertools.permutations(range(k))))
        tot = np.unique(cost[np.arange(k)[None, :], _perms[k]].sum(1))
        out[b] = len(tot) > 1 and tot[1] - tot[0] < gap
    return out


def _match_check(ops, oracle, mu, kap, w, vm, K, skip=None, check_assign=True):
    B, maxK = mu.shape
    md, kd, wd = (t.double().requires_grad_(True) for t in (mu, kap, w))
    l64, assign64 = oracle.match_loss(md, kd, wd, vm.double(), K, return_assignment=True)
    l64.sum().backward()
    mg, kg, wg = (t.clone().cuda().requires_grad_(True) for t in (mu, kap, w))
    lv = ops.match_loss(mg, kg, wg, vm.cuda(), K.cuda())
    assign = lv.grad_fn.assign.cpu().numpy()
    lv.sum().backward()
    keep = np.ones(B, bool) if skip is None else ~skip
    e = [_g5(_n(lv)[keep], _n(l64)[keep])] + [_g5(_n(a.grad)[keep], _n(r.grad)[keep]) for a, r in ((mg, md), (kg, kd), (wg, wd))]
    assert max(e) <= G5, e
    assert np.all(_n(lv)[K.numpy() == 0] == 0)
    for b in np.nonzero(keep)[0]:
        k = min(int(K[b]), maxK)
        assert np.all(assign[b, k:] == -1)
        assert sorted(assign[b, :k]) == list(range(k)), (b, assign[b])
        if check_assign:
            assert np.array_equal(assign[b, :k], assign64[b]), (b, assign[b], assign64[b])
    return e


@pytest.mark.parametrize("maxK", MATCH_MAXK)
def test_match_loss_every_width_and_block_edge(ops, oracle, maxK):
    """vm_match_loss_kernel at 256, 64, 28, 10 and 4 samples per workgroup, B on either side of one workgroup and ending inside the
    fourth; K_gt = 8 walks all 40,320 permutations on the packed nibbles.  Loss, the three gradients and the assignment itself
    against the float64 oracle (scipy's linear_sum_assignment)."""
    worst = np.zeros(4)
    for B in match_sizes(maxK):
        mu, kap, w, vm, K = match_case(maxK, B)
        skip = ambiguous(oracle, mu, kap, vm, K)
        assert skip.sum() <= 0.05 * B, (maxK, B, int(skip.sum()))
        worst = np.maximum(worst, _match_check(ops, oracle, mu, kap, w, vm, K, skip))
    _report(f"matching max_K={maxK}", loss=worst[0], dmu=worst[1], dkappa=worst[2], dw=worst[3])


def test_match_loss_duplicate_ground_truth_and_zero_weights(ops, oracle):
    """Identical ground-truth peaks: every assignment has the same total, so loss and gradients do not depend on the one taken (and
    the assignment is not compared).  Then sum w = 0: the loss is 0 / 1e-8 and d/dw = c / 1e-8."""
    mu, kap, w, vm, K = match_case(4, 21)
    vm[:, :, :2] = vm[:, :1, :2].clone()
    e = _match_check(ops, oracle, mu, kap, w, vm, K, check_assign=False)
    mu, kap, w, vm, K = match_case(3, 9)
    z = _match_check(ops, oracle, mu, kap, torch.zeros_like(w), vm, K, ambiguous(oracle, mu, kap, vm, K))
    _report("matching, duplicates / zero weights", dup=max(e), zero_w=max(z))


# ------------------------------------------------------------------------------------------------------------------------
# mvm head
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("B", [1, 64, 65])
def test_mvm_head_edges(ops, B, K):
    """test_mvm_head_forward_backward's reference and gate, at: direction norms 0 and 5e-8 (unit norm < 1e-3: fallback to (1, 0), no
    gradient), 2e-7 (just above the fallback, still r / eps), 9e-5 and 1.1e-4 (either side of the normalise eps 1e-4); softplus +
    1e-6 one float32 either side of kappa_max; temperature 0.05 with |pi_raw| up to 50 (logits +-1000).  The edges are planted
    slot by slot from the start of the batch; a batch smaller than the list carries its head."""
    f = np.float32
    temp, kmax = 0.05, 80.0
    g = torch.Generator().manual_seed(100 * B + K)
    pi = (torch.rand(B, K, generator=g) * 2 - 1) * 50
    mr = torch.randn(B, K, 2, generator=g) * 0.5
    kr = torch.randn(B, K, generator=g) * 3
    norms = [0.0, 5e-8, 2e-7, 9e-5, 1.1e-4]
    kraws = [np.nextafter(f(80), f(0)), 80.0, np.nextafter(f(80), f(90)), 19.5, 200.0]
    for s in range(min(B * K, 10)):
        b, k = divmod(s, K)
        th = 0.7 + 1.3 * s
        mr[b, k] = torch.tensor([math.cos(th), math.sin(th)]) * norms[s % 5]
        kr[b, k] = float(kraws[(s + s // 5) % 5])
    if B * K >= 2:
        pi.view(-1)[0], pi.view(-1)[1] = 50.0, -50.0
    mr = mr.reshape(B, 2 * K)
    pd, md, kd = (t.double().requires_grad_(True) for t in (pi, mr, kr))
    w_ref = torch.softmax(pd / float(f(temp)), -1)              # the op takes a float32 temperature
    raw = md.reshape(B, K, 2)
    unit = raw / raw.norm(dim=-1, keepdim=True).clamp_min(1e-4)
    c, s = unit[..., 0], unit[..., 1]
    small = torch.sqrt(c * c + s * s) < 1e-3
    mu_ref = torch.atan2(torch.where(small, torch.zeros_like(s), s), torch.where(small, torch.ones_like(c), c))
    kap_ref = (torch.nn.functional.softplus(kd) + 1e-6).clamp_max(kmax)
    gm, gk, gw = (torch.randn(B, K, generator=g).double() for _ in range(3))
    (mu_ref * gm + kap_ref * gk + w_ref * gw).sum().backward()
    pg, mg, kg = (t.clone().cuda().requires_grad_(True) for t in (pi, mr, kr))
    mu, kap, w = ops.mvm_head(pg, mg, kg, temp, kmax)
    (mu * gm.float().cuda() + kap * gk.float().cuda() + w * gw.float().cuda()).sum().backward()
    names = ("mu", "kappa", "w", "dpi", "dmu_raw", "dkappa_raw")
    errs = {}
    for name, got, ref in zip(names, (mu, kap, w, pg.grad, mg.grad, kg.grad), (mu_ref, kap_ref, w_ref, pd.grad, md.grad, kd.grad)):
        errs[name] = float((np.abs(_n(got) - _n(ref)) / np.maximum(1, np.abs(_n(ref)))).max())
    _report(f"mvm head B={B} K={K}", **errs)
    assert max(errs.values()) <= 2e-5, errs
    n_fb = min(B * K, 10)
    fb = [divmod(s, K) for s in range(n_fb) if s % 5 < 2]          # the fallback slots: mu = 0 and exactly no gradient
    for b, k in fb:
        assert float(mu[b, k]) == 0.0 and torch.all(mg.grad.view(B, K, 2)[b, k] == 0)
    for s in range(n_fb):                                          # past kappa_max: clamped, exactly no gradient
        b, k = divmod(s, K)
        if float(kr[b, k]) >= 80.0:
            assert float(kap[b, k]) == 80.0 and float(kg.grad[b, k]) == 0.0
        elif float(kr[b, k]) > 79.0:
            assert float(kap[b, k]) < 80.0 and float(kg.grad[b, k]) == float(gk[b, k].float())


# ------------------------------------------------------------------------------------------------------------------------
# fused vm tail
# ------------------------------------------------------------------------------------------------------------------------
def _offset_view(B, K):
    """A contiguous (B, K) tensor whose first element sits one float past a 16-byte boundary."""
    buf = torch.empty(B * K + 8, device="cuda")
    shift = 1 + ((16 - buf.data_ptr() % 16) % 16) // 4
    x = buf[shift:shift + B * K].view(B, K)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    return x


def _vm_tail_case(ops, B, K, misaligned=False, next_centres=None):
    """test_vm_fc_head_kl_loss_backward_equals_the_unfused_ops, its gates, at (B, K); returns the fused call's results."""
    torch.manual_seed(B * 131 + K)
    lin = nn.Linear(K, 2).cuda()
    x = torch.randn(B, K, device="cuda")
    if misaligned:
        x = _offset_view(B, K).copy_(x)
    mu_gt = (torch.rand(B, device="cuda") * 2 - 1) * 3.1
    kappa_gt = torch.rand(B, device="cuda") * 30 + 0.5
    xa = x.detach().requires_grad_(True)
    assert xa.data_ptr() == x.data_ptr()
    la = ops.vm_fc_head_kl_loss_backward(xa, lin, mu_gt, kappa_gt, next_centres=next_centres)
    ga = (lin.weight.grad.clone(), lin.bias.grad.clone(), xa.grad.clone())
    lin.zero_grad(set_to_none=True)
    xb = x.clone().requires_grad_(True)
    lb = ops.vm_head_kl_loss_backward(ops.fc_block(xb, lin, training=True), mu_gt, kappa_gt)
    gb = (lin.weight.grad.clone(), lin.bias.grad.clone(), xb.grad.clone())
    lin.zero_grad(set_to_none=True)
    e_unfused = [abs(float(la) - float(lb)) / max(1.0, abs(float(lb)))] + [_rel(_n(a), _n(b)) for a, b in zip(ga, gb)]
    assert e_unfused[0] <= 2e-6 and max(e_unfused[1:]) < 2e-5, e_unfused
    x64 = x.double().cpu().requires_grad_(True)
    W, b = lin.weight.detach().double().cpu().requires_grad_(True), lin.bias.detach().double().cpu().requires_grad_(True)
    o = x64 @ W.t() + b
    mu, kappa = torch.tanh(o[:, 0]) * np.pi, torch.nn.functional.softplus(o[:, 1])
    kq = kappa_gt.double().cpu()
    i0 = lambda k: torch.special.i0e(k) * torch.exp(k)
    a1 = torch.special.i1e(kappa) / torch.special.i0e(kappa)
    loss = (torch.log(i0(kq)) - torch.log(i0(kappa)) + a1 * (kappa - kq * torch.cos(mu - mu_gt.double().cpu()))).mean()
    loss.backward()
    e64 = [abs(float(la) - float(loss)) / max(1.0, abs(float(loss))), _rel(_n(ga[0]), _n(W.grad)), _rel(_n(ga[1]), _n(b.grad)),
           _rel(_n(ga[2]), _n(x64.grad))]
    assert e64[0] <= 1e-5 and max(e64[1:]) < 2e-5, e64
    return (la, *ga), lin, (x, mu_gt, kappa_gt), e64


VM_TAIL = [(1, 4, "lds"), (31, 8, "lds"), (33, 256, "lds"), (64, 192, "lds"), (65, 188, "lds"),      # x staged in LDS
           (4, 3073, "size"),                                                                        # B K > 12288: x read from memory
           (1, 1, "mod4"), (3, 5, "mod4"), (257, 7, "mod4"),                                         # B K % 4 != 0
           (32, 256, "align"),                                                                       # x not 16-byte aligned
           (8, 8000, "separate")]                                                                    # 2 K floats of W exceed the LDS budget


@pytest.mark.parametrize("B,K,why", VM_TAIL)
def test_vm_tail_shapes(ops, L, monkeypatch, B, K, why):
    """vm_fc_head_kl_step_kernel with x_in_lds on and off by each of its three conditions, the padded row loop (ic = min(i, B - 1))
    at B = 1, 31, 33, 65, 257, more than one 64-sample chunk, and the LDS refusal, which must take the separate launches."""
    fused = _Calls(monkeypatch, L, "pnpp_vm_fc_head_kl_step")
    _, _, _, e64 = _vm_tail_case(ops, B, K, misaligned=(why == "align"))
    assert fused.n == (0 if why == "separate" else 1)
    x_in_lds = B * K <= 12288 and (B * K) % 4 == 0 and why != "align"
    assert x_in_lds == (why == "lds")
    _report(f"vm tail B={B} K={K} ({why})", loss=e64[0], dW=e64[1], db=e64[2], dx=e64[3])


# ------------------------------------------------------------------------------------------------------------------------
# fused mvm tail
# ------------------------------------------------------------------------------------------------------------------------
def _mvm_lds_bytes(B, K, maxK):
    """o[B][4 mK] | ws[4 mK][K] | xs[B][K] | mu, kappa, weight [B][3 mK] | cost, gmu, gk [3][B][mK^2], float32"""
    return 4 * (B * 4 * maxK + 4 * maxK * K + B * K + 3 * B * maxK + 3 * B * maxK * maxK)


def _mvm_tail_case(ops, oracle, B, K, maxK, misaligned=False, next_centres=None):
    """test_mvm_heads_match_loss_backward_equals_the_unfused_ops, its gates, at (B, K, max_K)."""
    torch.manual_seed(B * 17 + K)
    heads = [nn.Linear(K, n).cuda() for n in (maxK, 2 * maxK, maxK)]
    x = torch.randn(B, K, device="cuda") * 0.5
    if misaligned:
        x = _offset_view(B, K).copy_(x)
    g = torch.Generator().manual_seed(B)
    Kgt = torch.randint(0, maxK + 1, (B,), generator=g)
    Kgt[0] = maxK                                        # (a batch of one must not be a batch without peaks: nothing to differentiate)
    vm = torch.zeros(B, maxK, 3)
    vm[:, :, 0] = (torch.rand(B, maxK, generator=g) * 2 - 1) * 3.1
    vm[:, :, 1] = torch.rand(B, maxK, generator=g) * 20 + 0.5
    vm[:, :, 2] = 1.0 / maxK
    temp, kmax = 0.7, 80.0
    xa = x.detach().requires_grad_(True)
    assert xa.data_ptr() == x.data_ptr()
    la, mu_a, kap_a, w_a = ops.mvm_heads_match_loss_backward(xa, *heads, vm.cuda(), Kgt.cuda(), temp, kmax, next_centres=next_centres,
                                                             outputs=True)
    ga = [p.grad.clone() for h in heads for p in (h.weight, h.bias)] + [xa.grad.clone()]
    for h in heads:
        h.zero_grad(set_to_none=True)
    xb = x.clone().requires_grad_(True)
    mu_b, kap_b, w_b = ops.mvm_head(*[ops.fc_block(xb, h, training=True) for h in heads], temp, kmax)
    lb = ops.match_loss(mu_b, kap_b, w_b, vm.cuda(), Kgt.cuda()).mean()
    lb.backward()
    gb = [p.grad.clone() for h in heads for p in (h.weight, h.bias)] + [xb.grad.clone()]
    for h in heads:
        h.zero_grad(set_to_none=True)
    assert not la.requires_grad and abs(float(la) - float(lb)) <= 2e-6 * max(1.0, abs(float(lb)))
    for a, b in ((mu_a, mu_b), (kap_a, kap_b), (w_a, w_b)):
        assert _rel(_n(a), _n(b)) < 2e-6
    for a, b in zip(ga, gb):
        assert _rel(_n(a), _n(b)) < 2e-5
    x64 = x.double().cpu().requires_grad_(True)
    P = {n: (h.weight.detach().double().cpu().requires_grad_(True), h.bias.detach().double().cpu().requires_grad_(True))
         for n, h in zip(("pi", "mu", "kappa"), heads)}
    raw = {n: x64 @ W.t() + b for n, (W, b) in P.items()}
    weight = torch.softmax(raw["pi"] / temp, -1)
    v = raw["mu"].view(B, maxK, 2)
    u = v / v.norm(dim=-1, keepdim=True).clamp_min(1e-4)
    mu64 = torch.atan2(u[..., 1], u[..., 0])
    kap64 = (torch.nn.functional.softplus(raw["kappa"]) + 1e-6).clamp_max(kmax)
    l64 = oracle.match_loss(mu64, kap64, weight, vm.double(), Kgt).mean()
    l64.backward()
    ref = [t.grad for n in ("pi", "mu", "kappa") for t in P[n]] + [x64.grad]
    e64 = [abs(float(la) - float(l64)) / max(1.0, abs(float(l64)))] + [_rel(_n(a), _n(r)) for a, r in zip(ga, ref)]
    assert e64[0] <= 1e-5 and max(e64[1:]) < 5e-5, e64
    return (la, mu_a, kap_a, w_a, *ga), heads, (x, vm, Kgt), e64


def _mvm_largest_B(K, maxK):
    B = 1
    while _mvm_lds_bytes(B + 1, K, maxK) <= 96 * 1024:
        B += 1
    return B


MVM_TAIL = [(1, 4, 4, 1), (31, 64, 4, 1), (33, 128, 8, 1), (65, 64, 4, 1),        # one launch
            (_mvm_largest_B(128, 8), 128, 8, 1),                                  # the largest batch the 96 KB hold at K = 128, max_K = 8
            (_mvm_largest_B(128, 8) + 1, 128, 8, 0),                              # one more: the separate launches
            (8, 30, 4, 0), (6, 64, 5, 0)]                                         # K % 4 != 0; a width that is not instantiated


@pytest.mark.parametrize("B,K,maxK,fused", MVM_TAIL)
def test_mvm_tail_shapes(ops, oracle, L, monkeypatch, B, K, maxK, fused):
    calls = _Calls(monkeypatch, L, "pnpp_mvm_fc_head_match_step")
    assert (_mvm_lds_bytes(B, K, maxK) <= 96 * 1024 and K % 4 == 0 and maxK in (4, 8)) == bool(fused)
    _, _, _, e64 = _mvm_tail_case(ops, oracle, B, K, maxK)
    assert calls.n == fused
    _report(f"mvm tail B={B} K={K} max_K={maxK} ({'one launch' if fused else 'separate'})", loss=e64[0], grads=max(e64[1:]))


def test_mvm_tail_misaligned_features_take_the_separate_launches(ops, oracle, L, monkeypatch):
    """The one-launch kernel stages x with 16-byte loads; a contiguous view at a 4-byte offset has to go the other way, not raise."""
    calls = _Calls(monkeypatch, L, "pnpp_mvm_fc_head_match_step")
    _, _, _, e64 = _mvm_tail_case(ops, oracle, 8, 64, 4, misaligned=True)
    assert calls.n == 0
    _report("mvm tail, misaligned x", loss=e64[0], grads=max(e64[1:]))


# ------------------------------------------------------------------------------------------------------------------------
# the centre draw riding in the tail launches
# ------------------------------------------------------------------------------------------------------------------------
def _with_and_without_rider(ops, run, N, Bs=3, npoint1=128, npoint2=32):
    """run(next_centres) -> tuple of tensors.  Same results with the rider as without; the ring holds the draw that
    ops.sample_random_dev2 makes from an equal counter; the counter went up by 2 and the ticket word is back at 0."""
    from pnpp_hip import sampling
    dev = torch.device("cuda", torch.cuda.current_device())
    counter = sampling._counter(dev)
    saved = counter.clone()
    try:
        start = torch.tensor([5, 0], dtype=torch.int64)
        plain = run(None)
        counter.copy_(start)
        ring = sampling.CentreRing(Bs, N, npoint1, npoint2, dev)
        seed, ctr, offset = ring.job()[:3]
        assert ctr is counter
        want = ops.sample_random_dev2(seed, counter, offset, Bs, N, npoint1, npoint1, npoint2)
        assert counter.tolist() == [7, 0]
        counter.copy_(start)
        ring.c1.fill_(-1), ring.c2.fill_(-1)
        ridden = run(ring.job())
        assert counter.tolist() == [7, 0]
        assert torch.equal(ring.c1, want[0]) and torch.equal(ring.c2, want[1])
        assert int(ring.c1.min()) >= 0 and int(ring.c1.max()) < N and int(ring.c2.max()) < npoint1
        assert len(plain) == len(ridden)
        for a, b in zip(plain, ridden):
            assert torch.equal(a, b)
    finally:
        counter.copy_(saved)


@pytest.mark.parametrize("N", [1024, 7167, 7168])
def test_vm_tail_with_the_riding_centre_draw(ops, L, monkeypatch, N):
    """(N + 1) * 8 bytes of candidate table: 8,200 (under the tail's own LDS), 57,344 (exactly the 56 KB) and 57,352 -- one past:
    the draw takes its own launch and the tail the plain one-launch form.  B = 16 samples in the tail, 3 clouds in the draw."""
    ride = _Calls(monkeypatch, L, "pnpp_vm_fc_head_kl_step_sample")
    alone = _Calls(monkeypatch, L, "pnpp_sample_random_dev2")
    _with_and_without_rider(ops, lambda job: _vm_tail_case(ops, 16, 64, next_centres=job)[0], N)
    assert (ride.n, alone.n) == ((1, 1) if N < 7168 else (0, 2))       # (the comparison draw is one of the stand-alone launches)


@pytest.mark.parametrize("N", [1024, 10000, 12288])
def test_mvm_tail_with_the_riding_centre_draw(ops, oracle, L, monkeypatch, N):
    """pnpp_mvm_fc_head_match_step with Bs > 0 (tools/bench_config.py's multi-peak step): candidate tables of 8,200 bytes, 80,008
    (more than the tail's own 29 KB: the launch takes the maximum) and 98,312 -- 8 past the 96 KB, which falls back."""
    fusedc = _Calls(monkeypatch, L, "pnpp_mvm_fc_head_match_step")
    alone = _Calls(monkeypatch, L, "pnpp_sample_random_dev2")
    _with_and_without_rider(ops, lambda job: _mvm_tail_case(ops, oracle, 16, 64, 4, next_centres=job)[0], N)
    assert alone.n == (1 if N < 12288 else 2) and fusedc.n == 2


# ------------------------------------------------------------------------------------------------------------------------
# Adam and the clip, straight through the C ABI
# ------------------------------------------------------------------------------------------------------------------------
F = lambda v: float(np.float32(v))      # the float32 the C ABI receives, as a float64
LR, B1, B2, EPS = F(1e-3), F(0.9), F(0.999), F(1e-8)
BIG_N = 2048 * 256 + 3                  # past the grid cap of 2048 workgroups x 256 threads: the grid-stride loop wraps


def _adam_buffers(n, seed):
    """Gradients log-uniform in magnitude over [1e-12, 1e3] with random signs, every 11th exactly zero; moments carried in, m with
    the gradient's sign except every 7th element (opposite: b1 m + (1 - b1) g cancels there); every 22nd element has zero
    gradient AND zero moments (p must not move).  p of order 1."""
    r = np.random.default_rng(seed)
    g = (10.0 ** r.uniform(-12, 3, n) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    i = np.arange(n)
    g[i % 11 == 0] = 0.0
    sign = np.where(g != 0, np.sign(g), r.choice([-1.0, 1.0], n)) * np.where(i % 7 == 3, -1.0, 1.0)
    m = (sign * 10.0 ** r.uniform(-8, 1, n)).astype(np.float32)
    v = ((m.astype(np.float64) ** 2) * 10.0 ** r.uniform(0, 2, n)).astype(np.float32)
    still = i % 22 == 0
    m[still], v[still] = 0.0, 0.0
    p = r.normal(0, 1, n).astype(np.float32)
    return p, g, m, v, still


def _adam_ref(p, g, m, v, step, gscale, coef=1.0):
    """torch.optim.Adam (no amsgrad, no weight decay) in float64 on the float32 buffers: step_size = lr / bc1,
    denom = sqrt(v) / sqrt(bc2) + eps."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    gi = g * (gscale * coef)
    t1, t2 = B1 * m, (1.0 - B1) * gi
    m2 = t1 + t2
    v2 = B2 * v + (1.0 - B2) * gi * gi
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    denom = np.sqrt(v2) / math.sqrt(bc2) + EPS
    dp = (LR / bc1) * m2 / denom
    return p - dp, m2, v2, dp, np.abs(t1) + np.abs(t2), (LR / bc1) / denom


def _adam_check(tag, out, ref, p0, kg=0):
    """Bounds from counting float32 roundings (U = 2^-24 each), kg of them in g * grad_scale * clip (0: the factor is 1 or 0.5).
    m = b1 m + (1 - b1) g: two products and a sum, three roundings -> 4 U of |b1 m| + |(1 - b1) g| (that is |m| itself unless the
    two terms cancel), + kg U for g's own error.  v likewise, 4 U + 2 kg U (g enters squared).  p: one ulp of p for the final
    subtraction + 1e-6 |dp| (= 16.8 U) for the seven roundings of lr/bc1 * m / (sqrt(v) / sqrt(bc2) + eps) on top of m's four
    and half of v's four, + 2 kg U |dp|; where the two terms of m cancel, what m's allowance exceeds (4 + kg) U |m| by is carried
    through step_size / denom (zero everywhere else)."""
    pg, mg, vg = (a.astype(np.float64) for a in out)
    p_ref, m_ref, v_ref, dp, mscale, gain = ref
    m_allow = (4 + kg) * U * mscale
    rm = np.abs(mg - m_ref) / np.maximum(m_allow, 1e-300)
    rv = np.abs(vg - v_ref) / np.maximum((4 + 2 * kg) * U * v_ref, 1e-300)
    ulp = np.spacing(np.maximum(np.abs(p0), np.abs(p_ref)).astype(np.float32)).astype(np.float64)
    m_excess = np.maximum(m_allow - (4 + kg) * U * np.abs(m_ref), 0.0)
    rp = np.abs(pg - p_ref) / (ulp + (1e-6 + 2 * kg * U) * np.abs(dp) + gain * m_excess)
    sub = float(np.finfo(np.float32).tiny)       # results below the normal range carry an absolute 2^-149 instead
    rm[np.abs(m_ref) < sub], rv[v_ref < sub] = 0.0, 0.0
    w = (float(rm.max()), float(rv.max()), float(rp.max()))
    assert max(w) <= 1.0, (tag, w)
    return w


def _dev(a):
    return torch.from_numpy(a.copy()).cuda()


@pytest.mark.parametrize("n", [1, 255, 256, 257, BIG_N])
def test_adam_step_against_float64(L, n):
    """pnpp_adam_step / _zero and pnpp_adam_step_dev on hand-made buffers: eps placement (gradients from 1e-12 up, exact zeros),
    bias correction at steps 1, 2, 1000 and 100000, the wrap of the grid-stride loop, grad_scale, the folded zero_grad."""
    lib = L.lib()
    s = torch.cuda.current_stream().cuda_stream
    p0, g0, m0, v0, still = _adam_buffers(n, n)
    combos = list(itertools.product((1, 2, 1000, 100000), (1.0, 0.5), (0, 1)))
    if n == BIG_N:
        combos = [c for i, c in enumerate(combos) if i % 4 in (0, 3)]      # every step count, each scale and each zeroing
    worst = np.zeros(3)
    for step, gscale, zero in combos:
        ref = _adam_ref(p0, g0, m0, v0, step, gscale)
        # host step count
        p, g, m, v = (_dev(a) for a in (p0, g0, m0, v0))
        fn = lib.pnpp_adam_step_zero if zero else lib.pnpp_adam_step
        L.check(fn(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, LR, B1, B2, EPS, gscale, s))
        out = [t.cpu().numpy() for t in (p, m, v)]
        worst = np.maximum(worst, _adam_check(("host", n, step, gscale, zero), out, ref, p0))
        assert np.array_equal(g.cpu().numpy(), np.zeros_like(g0) if zero else g0)
        assert np.array_equal(out[0][still], p0[still])
        # device step count, seeded at step - 1 ... so that it applies `step`; a second seed at `step` is the issue's own count
        for seeded in ({step - 1, step} if n != BIG_N else {step - 1}):
            refd = ref if seeded == step - 1 else _adam_ref(p0, g0, m0, v0, step + 1, gscale)
            p, g, m, v = (_dev(a) for a in (p0, g0, m0, v0))
            state = torch.tensor([seeded, 0], dtype=torch.int64, device="cuda")
            L.check(lib.pnpp_adam_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(), LR, B1, B2, EPS,
                                           gscale, zero, s))
            outd = [t.cpu().numpy() for t in (p, m, v)]
            worst = np.maximum(worst, _adam_check(("dev", n, seeded, gscale, zero), outd, refd, p0))
            assert state.tolist() == [seeded + 1, 0]
            assert np.array_equal(g.cpu().numpy(), np.zeros_like(g0) if zero else g0)
            assert np.array_equal(outd[0][still], p0[still])
    _report(f"Adam n={n} (fraction of the derived bound)", m=worst[0], v=worst[1], p=worst[2])


@pytest.mark.parametrize("n", [257, BIG_N])
def test_adam_clip_against_float64(L, n):
    """pnpp_adam_step_clip / _dev_clip: coefficient min(1, max_norm / (norm * grad_scale + 1e-6)) (torch.nn.utils.clip_grad_norm_)
    with the norm below, above and within 1e-6 of max_norm, and norm 0.  The kernel forms the coefficient in float32 -- cast of
    the norm, the sum, the quotient, the product with grad_scale, then g times it: kg = 5 roundings in every g, 0 where it is 1."""
    lib = L.lib()
    s = torch.cuda.current_stream().cuda_stream
    p0, g0, m0, v0, still = _adam_buffers(n, 7 * n)
    scratch = torch.empty(1024 * 8, dtype=torch.uint8, device="cuda")
    worst = np.zeros(3)
    for gscale, (case, zero, step) in itertools.product((1.0, 0.5), (("above", 0, 1), ("below", 1, 1000), ("near-", 0, 2), ("near+", 1, 2),
                                                                     ("zero", 0, 100000))):
        gin = np.zeros_like(g0) if case == "zero" else g0
        g = _dev(gin)
        ss = torch.zeros(1, dtype=torch.float64, device="cuda")
        L.check(lib.pnpp_sumsq(g.data_ptr(), n, ss.data_ptr(), scratch.data_ptr(), scratch.numel(), s))
        norm = math.sqrt(math.fsum((gin.astype(np.float64) ** 2).tolist())) * gscale
        assert abs(math.sqrt(float(ss)) * gscale - norm) <= 1e-12 * norm
        max_norm = {"above": F(norm * 0.37), "below": F(norm * 2.5), "near-": F(norm * (1 - 4e-7)), "near+": F(norm * (1 + 4e-7)),
                    "zero": F(1.0)}[case]
        coef = min(1.0, max_norm / (norm + 1e-6))
        assert (coef < 0.5) if case == "above" else (coef == 1.0) if case in ("below", "zero") else (1 - 2e-6 < coef <= 1.0)
        kg = 0 if case in ("below", "zero") else 5
        for dev in (0, 1):
            ref = _adam_ref(p0, gin, m0, v0, step, gscale, coef)
            p, g, m, v = (_dev(a) for a in (p0, gin, m0, v0))
            if dev:
                state = torch.tensor([step - 1, 0], dtype=torch.int64, device="cuda")
                L.check(lib.pnpp_adam_step_dev_clip(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(), LR, B1, B2,
                                                    EPS, gscale, ss.data_ptr(), max_norm, zero, s))
                assert state.tolist() == [step, 0]
            else:
                L.check(lib.pnpp_adam_step_clip(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, LR, B1, B2, EPS, gscale,
                                                ss.data_ptr(), max_norm, zero, s))
            out = [t.cpu().numpy() for t in (p, m, v)]
            worst = np.maximum(worst, _adam_check((case, n, gscale, dev), out, ref, p0, kg))
            assert np.array_equal(g.cpu().numpy(), np.zeros_like(g0) if zero else gin)
            assert np.array_equal(out[0][still], p0[still])
    _report(f"Adam + clip n={n} (fraction of the derived bound)", m=worst[0], v=worst[1], p=worst[2])


@pytest.mark.parametrize("n", [1, 257, 1024 * 256 + 5])
def test_sumsq_against_float64(L, n):
    """pnpp_sumsq past its grid cap (1024 workgroups x 256 threads), values up to 1e30.  A product of two float32 is exact in
    float64, so only the order of the sum differs from the exactly rounded math.fsum: relative 1e-12 (n * 2^-53 = 3e-11 is the
    worst case of ANY order over 262,149 positive terms; a tree of 1024 x 256 partial sums stays under log2 of that)."""
    r = np.random.default_rng(n)
    x = (10.0 ** r.uniform(-20, 30, n) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    if n > 1:
        x[1] = 0.0
    ref = math.fsum((x.astype(np.float64) ** 2).tolist())
    xd = _dev(x)
    out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    nb = min((n + 255) // 256, 1024)
    scratch = torch.empty(nb * 8, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L.check(L.lib().pnpp_sumsq(xd.data_ptr(), n, out.data_ptr(), scratch.data_ptr(), scratch.numel(), s))
    e = abs(float(out) - ref) / ref
    _report(f"sumsq n={n}", rel=e)
    assert e <= 1e-12
    # uniform values: every element counted exactly once across the wrap
    xd.fill_(3.0)
    L.check(L.lib().pnpp_sumsq(xd.data_ptr(), n, out.data_ptr(), scratch.data_ptr(), scratch.numel(), s))
    assert float(out) == 9.0 * n
    if nb > 1:
        with pytest.raises(RuntimeError):
            L.check(L.lib().pnpp_sumsq(xd.data_ptr(), n, out.data_ptr(), scratch.data_ptr(), (nb - 1) * 8, s))


# ------------------------------------------------------------------------------------------------------------------------
# soft-label cross entropy, log-softmax + NLL
# ------------------------------------------------------------------------------------------------------------------------
def _wild_logits(B, Cc, g):
    x = 3.0 * torch.randn(B, Cc, generator=g)
    x[0, 0] = 1e4
    if Cc > 1:
        x[0, 1] = -1e4
        x[B // 2, Cc - 1] = -1e4
    if B > 2:
        x[B - 1] = -1e4
        x[B - 1, Cc // 2] = 1e4
    return x


@pytest.mark.parametrize("Cc", [1, 8, 40, 65])
@pytest.mark.parametrize("B", [1, 64, 65])
def test_soft_ce_and_log_softmax_nll_wild_rows(ops, B, Cc):
    """Logits of +-1e4 in one row; soft targets with exact zeros that do not sum to 1 (the gradient is softmax * sum p - p).
    Gates of test_soft_ce and test_log_softmax_nll_loss_vs_float64: rtol 1e-5, atol 1e-6 against float64 log_softmax."""
    g = torch.Generator().manual_seed(77 * B + Cc)
    x = _wild_logits(B, Cc, g)
    p = torch.rand(B, Cc, generator=g) * 1.7
    p[torch.rand(B, Cc, generator=g) < 0.3] = 0.0
    p[0, 0] = 0.0
    t = torch.randint(0, Cc, (B,), generator=g)
    up = torch.randn(B, Cc, generator=g)
    xd = x.double().requires_grad_(True)
    yd = torch.log_softmax(xd, 1)
    ce64 = -(p.double() * yd).sum(1)
    nll64 = torch.nn.functional.nll_loss(yd, t)
    refs = [ce64, torch.autograd.grad(ce64.sum(), xd, retain_graph=True)[0], yd, nll64,
            torch.autograd.grad(nll64, xd, retain_graph=True)[0], torch.autograd.grad((yd * up.double()).sum(), xd)[0]]
    xg = x.cuda().requires_grad_(True)
    ce = ops.soft_ce(xg, p.cuda())
    y = ops.log_softmax(xg)
    nll = ops.nll_loss(y, t.cuda())
    gots = [ce, torch.autograd.grad(ce.sum(), xg)[0], y, nll, torch.autograd.grad(nll, xg, retain_graph=True)[0],
            torch.autograd.grad((y * up.cuda()).sum(), xg)[0]]
    names = ("soft_ce", "d soft_ce", "log_softmax", "nll", "d nll", "d log_softmax")
    errs = {}
    for name, got, ref in zip(names, gots, refs):
        got, ref = _n(got), _n(ref)
        errs[name] = float((np.abs(got - ref) / (1e-6 + 1e-5 * np.abs(ref))).max())
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-6), name
    _report(f"CE / NLL B={B} C={Cc} (fraction of atol 1e-6 + rtol 1e-5)", **errs)
