"""tests/golden/tail_edges.npz (oracle/make_tail_golden.py: mpmath, 60 digits) pinned on the CPU: it regenerates byte for byte
where mpmath is installed, and it agrees with the three other statements of the same formulas this repository holds -- the
float64 oracle (oracle.restatement.kl_single / kl_multi, ATen's Cephes series), the float64 captures of the reference's own
functions (tests/golden/kl.npz) and the float64 formulas of csrc/vonmises.h restated here and rounded once to float32."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import make_tail_golden as gen
from oracle import restatement as R

G5 = 1e-5          # the suite's gate for heads and losses: |got - ref| <= G5 * max(1, |ref|)
F64_GATE = 1e-9    # float64 restatements against mpmath: seven digits under G5, four over what the Cephes series deliver


def _err(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(1.0, np.abs(ref))


def test_fixture_regenerates_byte_for_byte(golden):
    mpmath = pytest.importorskip("mpmath")
    assert mpmath.mp is not None
    fresh = gen.compute()
    g = golden("tail_edges.npz")
    assert sorted(g.files) == sorted(fresh)
    for k, v in fresh.items():
        assert g[k].dtype == v.dtype and g[k].shape == v.shape, k
        assert g[k].tobytes() == v.tobytes(), k
    with open(gen.DEFAULT, "rb") as f:
        assert f.read() == gen.npz_bytes(fresh)


def test_fixture_covers_the_sweep(golden):
    g = golden("tail_edges.npz")
    kp, kq, d = gen.sweep()
    inp = g["inputs"]
    assert inp.dtype == np.float32 and inp.shape == (len(kp) * len(kq) * len(d), 4)
    assert set(inp[:, 1].tolist()) == set(kp.tolist()) and set(inp[:, 3].tolist()) == set(kq.tolist())
    assert set((inp[:, 0] - inp[:, 2]).tolist()) == set(d.tolist())
    one, five = np.float32(1e-6), np.float32(500.0)
    for edge in (one, five):    # the neighbours of the thresholds, not their float32 roundings
        assert edge not in inp[:, 1]
        assert np.nextafter(edge, np.float32(0)) in inp[:, 1] and np.nextafter(edge, np.float32(1e9)) in inp[:, 1]
    assert np.float32(8.0) in inp[:, 1] and np.nextafter(np.float32(8.0), np.float32(9)) in inp[:, 1]
    assert np.isfinite(g["single"]).all() and np.isfinite(g["multi"]).all() and np.isfinite(g["bessel"]).all()
    assert os.path.getsize(gen.DEFAULT) < 64 * 1024


def test_fixture_vs_float64_oracle(golden):
    """oracle.restatement in float64 wherever its unscaled i0 is finite (kappa <= 500.00003 here; i0 overflows past ~713).
    The multi-peak d/d kappa_p leaves out kappa_p = 499.99997: autograd of the oracle's log(i0q / i0p) goes through i0p^2, which
    overflows float64 from kappa ~ 357 on, and loses that term (with kappa_q = 0 it returns 1.0 where the derivative is 1.0e-3)."""
    g = golden("tail_edges.npz")
    c = torch.from_numpy(g["inputs"]).double()
    for name, fn, keep in (("single", R.kl_single, c[:, 1] <= 600.0), ("multi", R.kl_multi, torch.ones(len(c), dtype=torch.bool))):
        cc = c[keep]
        a, b = cc[:, 0].clone().requires_grad_(True), cc[:, 1].clone().requires_grad_(True)
        v = fn(a, b, cc[:, 2], cc[:, 3])
        v.sum().backward()
        got = np.stack([v.detach().numpy(), a.grad.numpy(), b.grad.numpy()], 1)
        e = _err(got, g[name][keep.numpy()])
        dk_ok = ((cc[:, 1] <= 350.0) | (cc[:, 1] > 500.0)).numpy() if name == "multi" else np.ones(len(cc), bool)
        print(f"  {name}: {int(keep.sum())} rows, worst error vs mpmath {e[:, 0].max():.2e} {e[:, 1].max():.2e} {e[dk_ok, 2].max():.2e}")
        assert np.all(e[:, :2] <= F64_GATE) and np.all(e[dk_ok, 2] <= F64_GATE), name
        assert int((~dk_ok).sum()) == (5 * 7 if name == "multi" else 0)
    assert int((c[:, 1] <= 600.0).sum()) == len(c) - 2 * 5 * 7     # only kappa_p = 1e4 and 1e6 are out of the oracle's reach


def test_fixture_vs_reference_captures(golden):
    """Rows of tests/golden/kl.npz (the reference's own functions in float64) that the sweep meets: kl.npz holds mu_p = 0,
    mu_q = 3.1, the sweep mu_p = 3.1, mu_q = 0 -- the same |mu_p - mu_q|, so the same KL and d/d kappa and the negated d/d mu."""
    g, k = golden("tail_edges.npz"), golden("kl.npz")
    mine = {(float(r[1]), float(r[3]), float(r[0] - r[2])): i for i, r in enumerate(g["inputs"])}
    n = 0
    for j, r in enumerate(k["single_in"]):
        i = mine.get((float(r[1]), float(r[3]), float(r[2] - r[0])))      # my mu_p - mu_q = -(theirs)
        if i is None:
            continue
        n += 1
        flip = np.array([1.0, -1.0, 1.0])
        for name in ("single", "multi"):
            ref = g[name][i]
            assert np.all(_err(k[name + "_f64"][j] * flip, ref) <= F64_GATE), (name, r)
    assert n >= 12, n


def _kernel_formulas(c):
    """kl_single_eval / kl_multi_eval of csrc/vonmises.h in float64 (torch.special.i0e / i1e are the same Cephes series)."""
    mp_, kp_raw, mq, kq_raw = (c[:, i] for i in range(4))
    i0e, i1e = torch.special.i0e, torch.special.i1e
    log_i0 = lambda k: k + torch.log(i0e(k))
    ratio = lambda k: i1e(k) / i0e(k)
    prime = lambda k, a: torch.where(k > 1e-8, 1.0 - a * a - a / k.clamp_min(1e-300), torch.full_like(k, 0.5))
    d = mp_ - mq
    a = ratio(kp_raw)
    base = log_i0(kq_raw) - log_i0(kp_raw)
    small = kp_raw <= 1e-6
    single = torch.stack([torch.where(small, base, base + kp_raw * a - kq_raw * a * torch.cos(d)),
                          torch.where(small, torch.zeros_like(a), kq_raw * a * torch.sin(d)),
                          torch.where(small, -a, prime(kp_raw, a) * (kp_raw - kq_raw * torch.cos(d)))], 1)
    kp, kq = kp_raw.clamp(1e-6, 500.0), kq_raw.clamp(1e-6, 500.0)
    w = torch.fmod(mp_ - mq + math.pi, 2 * math.pi)
    w = torch.where(w < 0, w + 2 * math.pi, w) - math.pi
    a = ratio(kp)
    gate = (kp_raw >= 1e-6) & (kp_raw <= 500.0)
    multi = torch.stack([log_i0(kq) - log_i0(kp) + a * (kp - kq * torch.cos(w)), a * kq * torch.sin(w),
                         torch.where(gate, prime(kp, a) * (kp - kq * torch.cos(w)), torch.zeros_like(a))], 1)
    return single, multi


def test_kernel_formulas_meet_g5_with_room(golden):
    """What the GPU tests rely on: the kernels' float64 formulas, rounded once to float32, sit at float32 rounding from mpmath
    over the whole sweep -- the cancellation of A' = 1 - A^2 - A/k at kappa = 1e6 included -- so G5 has two orders of room."""
    g = golden("tail_edges.npz")
    single, multi = _kernel_formulas(torch.from_numpy(g["inputs"]).double())
    for name, got in (("single", single), ("multi", multi)):
        e = _err(got.float().double().numpy(), g[name])
        print(f"  {name}: worst error of the kernel's formulas, rounded to float32, vs mpmath {e.max(0)}")
        assert np.all(e <= 1e-7), name       # 2^-24 = 6e-8 is one float32 rounding
    # and the Bessel pieces on their own, in float64 (before any rounding to float32)
    k = torch.from_numpy(g["bessel_kappa"]).double()
    a = torch.special.i1e(k) / torch.special.i0e(k)
    got = np.stack([(k + torch.log(torch.special.i0e(k))).numpy(), a.numpy(),
                    torch.where(k > 1e-8, 1.0 - a * a - a / k.clamp_min(1e-300), torch.full_like(k, 0.5)).numpy()], 1)
    e = _err(got, g["bessel"])
    print(f"  log I0, A, A': worst float64 error vs mpmath {e.max(0)}")
    assert np.all(e <= F64_GATE)
    assert G5 / 1e-7 >= 100


def test_matching_seeds_leave_the_reference_unambiguous(oracle):
    """The seeded cases of tests/test_gpu_tail_edges.py, on the reference alone: no sample's best and second-best assignment lie
    within 1e-4 of each other, so the GPU test's 5 % skip cap has all its room (continuous draws: the expected count is 0)."""
    import test_gpu_tail_edges as T
    for maxK in T.MATCH_MAXK:
        sizes = T.match_sizes(maxK)
        assert len(sizes) == 5 and sizes[1] + 1 == sizes[2] == 256 // (maxK * maxK)
        for B in sizes:
            mu, kap, w, vm, K = T.match_case(maxK, B)
            assert set(K.tolist()) <= set(range(maxK + 1)) | {maxK + 3}
            if B > maxK + 2:
                assert set(K.tolist()) == set(range(maxK + 1)) | {maxK + 3}
            assert int(T.ambiguous(oracle, mu, kap, vm, K).sum()) == 0, (maxK, B)


def test_adam_restatement_is_torch_optim_adam():
    """The float64 restatement the GPU test holds pnpp_adam_step* against IS torch.optim.Adam: one step of torch's own optimiser
    in float64 from the same carried-in moments and step count."""
    import test_gpu_tail_edges as T
    p0, g0, m0, v0, _ = T._adam_buffers(1000, 3)
    for step in (1, 2, 1000):
        P = torch.nn.Parameter(torch.from_numpy(p0).double())
        opt = torch.optim.Adam([P], lr=T.LR, betas=(T.B1, T.B2), eps=T.EPS)
        P.grad = torch.from_numpy(g0).double()
        opt.step()                                              # creates the state
        st = opt.state[P]
        P.data = torch.from_numpy(p0).double()
        st["exp_avg"], st["exp_avg_sq"] = torch.from_numpy(m0).double(), torch.from_numpy(v0).double()
        st["step"] = torch.tensor(float(step - 1))
        opt.step()
        ref = T._adam_ref(p0, g0, m0, v0, step, 1.0)
        for got, want in ((P.data, ref[0]), (st["exp_avg"], ref[1]), (st["exp_avg_sq"], ref[2])):
            assert np.all(np.abs(got.numpy() - want) <= 1e-14 * np.maximum(1.0, np.abs(want)))
