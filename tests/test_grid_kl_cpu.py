"""The mixture KL on the decode grid without a GPU: the float64 restatement (tests/grid_kl_ref.py) against the closed-form KL of two
von-Mises densities and against torch autograd of the formula, its invariances, the loophole of match_loss that it closes, the
mu_init switch of the model, the training script's defaults, and every refusal of the two C entry points (they come before any launch).
"""
import math

import numpy as np
import pytest
import torch

import grid_kl_ref as R


@pytest.fixture(scope="module")
def h():
    from pnpp_hip import build, _lib
    build.build()
    return _lib.lib()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
KAPPAS = (1e-6, 0.5, 8.0, 80.0, 500.0)


@pytest.mark.parametrize("kq", KAPPAS)
@pytest.mark.parametrize("kp", KAPPAS)
def test_one_component_equals_closed_form(kp, kq):
    """KL(vM_gt || vM_pred) in closed form is kl_von_mises with the ground truth first; the rectangle rule on 359 points is exact for
    every kappa the head can produce.  Gate 1e-11 absolute (measured <= 6e-14)."""
    import train_multi_peaks_vonMises_KL as T
    mu_gt, mu_p = 0.3, -0.2
    gt = np.array([[mu_gt, kq, 1.0]])
    loss = R.sample([mu_p], [kp], [1.0], gt, 1, 360)[0]
    f = lambda x: torch.tensor(x, dtype=torch.float64)
    want = float(T.kl_von_mises(f(mu_gt), f(kq), f(mu_p), f(kp)))
    print(f"kappa_pred={kp} kappa_gt={kq} grid={loss:.15g} closed={want:.15g} diff={abs(loss - want):.3g}")
    assert abs(loss - want) <= 1e-11


def _torch_formula(mu, kappa, weight, gt, num):
    """The definition in torch float64, for autograd: all components live, kappa inside the clamp."""
    G = num - 1
    th = torch.arange(G, dtype=torch.float64) * (2.0 * math.pi / G)
    def log_mix(m, k, w):
        lv = k[:, None] * (torch.cos(th[None, :] - m[:, None]) - 1.0) - torch.log(2.0 * math.pi * torch.special.i0e(k))[:, None]
        return torch.logsumexp(lv + torch.log(w)[:, None], dim=0)
    v = gt[:, 2] / gt[:, 2].sum()
    lq, lp = log_mix(gt[:, 0], gt[:, 1], v), log_mix(mu, kappa, weight)
    return (2.0 * math.pi / G) * torch.sum(torch.exp(lq) * (lq - lp))


@pytest.mark.parametrize("K,Kg,num,seed", [(1, 1, 360, 0), (2, 2, 360, 1), (4, 2, 360, 2), (4, 4, 258, 3), (8, 3, 360, 4), (8, 8, 9, 5)])
def test_gradients_equal_autograd(K, Kg, num, seed):
    g = torch.Generator().manual_seed(seed)
    mu = ((torch.rand(K, generator=g, dtype=torch.float64) * 2 - 1) * math.pi).requires_grad_(True)
    kappa = (torch.rand(K, generator=g, dtype=torch.float64) * 60 + 0.01).requires_grad_(True)
    weight = (torch.rand(K, generator=g, dtype=torch.float64) + 0.05).requires_grad_(True)   # not normalised: the loss takes them as given
    gt = torch.zeros(K, 3, dtype=torch.float64)
    gt[:, 0] = (torch.rand(K, generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    gt[:, 1] = torch.rand(K, generator=g, dtype=torch.float64) * 60 + 0.01
    gt[:, 2] = torch.rand(K, generator=g, dtype=torch.float64) + 0.1
    want = _torch_formula(mu, kappa, weight, gt[:Kg], num)
    want.backward()
    want = want.detach()
    loss, dmu, dk, dw = R.sample(mu.detach().numpy(), kappa.detach().numpy(), weight.detach().numpy(), gt.numpy(), Kg, num)
    assert abs(loss - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    for name, got, ref in (("dmu", dmu, mu.grad), ("dkappa", dk, kappa.grad), ("dweight", dw, weight.grad)):
        err = np.abs(got - ref.numpy()).max() / max(float(ref.abs().max()), 1e-300)
        print(f"K={K} Kg={Kg} num={num} {name}: {err:.3g} of max")
        assert err <= 1e-12, name


def test_identical_mixtures_give_zero():
    rng = np.random.RandomState(3)
    for K in (1, 2, 4, 8):
        gt = np.stack((rng.uniform(-math.pi, math.pi, K), rng.choice([0.5, 8.0, 80.0, 500.0], K), rng.uniform(0.1, 1.0, K)), axis=1)
        gt[:, 2] /= gt[:, 2].sum()
        loss, dmu, dk, dw = R.sample(gt[:, 0], gt[:, 1], gt[:, 2], gt, K, 360)
        assert abs(loss) <= 1e-12
        assert np.abs(dmu).max() <= 1e-9 and np.abs(dk).max() <= 1e-9      # a minimum in mu and kappa (sums of O(kappa) terms)
        assert np.abs(dw + 1.0).max() <= 1e-12                             # d/dw_i = -int q vM_i / p = -1 where p = q


def test_permutations_change_nothing():
    rng = np.random.RandomState(5)
    K = 4
    mu, kappa, w = rng.uniform(-3, 3, K), rng.uniform(0.1, 90, K), rng.uniform(0.1, 1, K)
    gt = np.stack((rng.uniform(-3, 3, K), rng.uniform(0.1, 90, K), rng.uniform(0.1, 1, K)), axis=1)
    base = R.sample(mu, kappa, w, gt, K, 360)
    for _ in range(6):
        p, q = rng.permutation(K), rng.permutation(K)
        got = R.sample(mu[p], kappa[p], w[p], gt[q], K, 360)
        assert abs(got[0] - base[0]) <= 1e-13
        for a, b in zip(got[1:], base[1:]):
            assert np.abs(a - b[p]).max() <= 1e-13 * max(1.0, np.abs(b).max())


def test_loophole_of_match_loss_is_closed():
    """The first K_gt predicted components copy the ground truth, so match_loss = sum w_i * 0 / sum w_i = 0 whatever weight they
    carry; 0.9 of the predicted mass lies on two flat extra components, and the mixture KL charges for it."""
    mu, kappa, weight, gt, kg = R.loophole_row()
    loss = R.sample(mu, kappa, weight, gt, kg, 360)[0]
    print(f"loophole row: {loss:.6f}")
    assert loss > 0.5
    assert abs(loss - 0.600) < 5e-3


def test_skips_and_clamps():
    mu, kappa, weight, gt, kg = R.loophole_row()
    zero = R.sample(mu, kappa, weight, gt, 0, 360)
    assert zero[0] == 0.0 and all(np.all(g == 0.0) for g in zero[1:])
    none = gt.copy()
    none[:, 2] = 0.0
    assert R.sample(mu, kappa, weight, none, 2, 360)[0] == 0.0
    assert R.sample(mu, kappa, weight, gt, 9, 360)[0] == R.sample(mu, kappa, weight, gt, 4, 360)[0]    # K_gt > max_K is clamped
    big = kappa.copy()
    big[0] = 600.0
    at_clamp = kappa.copy()
    at_clamp[0] = 500.0
    a, b = R.sample(mu, big, weight, gt, kg, 360), R.sample(mu, at_clamp, weight, gt, kg, 360)
    assert a[0] == b[0] and a[2][0] == 0.0 and b[2][0] != 0.0            # the clamped value gets no gradient
    w0 = weight.copy()
    w0[2] = 0.0
    got = R.sample(mu, kappa, w0, gt, kg, 360)
    assert got[1][2] == 0.0 and got[2][2] == 0.0 and got[3][2] < 0.0       # skipped in p; d/dw is defined at w = 0


def test_descent_on_the_restatement():
    """What the GPU descent test repeats in float32: 40 steps of plain gradient descent from the spread start, strictly decreasing."""
    losses = R.descent()
    print(f"descent: {losses[0]:.4f} -> {losses[-1]:.4f}, smallest step {min(a - b for a, b in zip(losses, losses[1:])):.3g}")
    assert abs(losses[0] - 0.7307) < 5e-4 and abs(losses[39] - 0.7036) < 5e-4   # the 40 values a 40-step loop sees
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert min(a - b for a, b in zip(losses, losses[1:])) > 1e-4           # far above float32 resolution


def test_head_restatement_against_torch():
    """R.head is the model's head: softmax(pi / temp), atan2 of the normalised direction, softplus + 1e-6 clamped."""
    g = torch.Generator().manual_seed(9)
    pi, mr, kr = (torch.randn(n, generator=g, dtype=torch.float64) for n in (4, 8, 4))
    kr[0] = 90.0
    mu, kappa, w = R.head(pi.numpy(), mr.numpy(), kr.numpy(), 0.7, 80.0)
    u = torch.nn.functional.normalize(mr.view(4, 2), dim=1, eps=1e-4)
    assert np.abs(mu - torch.atan2(u[:, 1], u[:, 0]).numpy()).max() < 1e-15
    assert np.abs(w - torch.softmax(pi / 0.7, 0).numpy()).max() < 1e-15
    assert np.abs(kappa - torch.clamp_max(torch.nn.functional.softplus(kr) + 1e-6, 80.0).numpy()).max() < 1e-14
    assert R.head(pi.numpy(), np.zeros(8), kr.numpy(), 0.7, 80.0)[0].tolist() == [0.0] * 4


# ---- the model's switch and the script's defaults -------------------------------------------------------------------------------------
def test_mu_init():
    from models.pointnet_pp_mvM import PointNetPPMvM
    torch.manual_seed(0)
    ref = PointNetPPMvM()
    torch.manual_seed(0)
    named = PointNetPPMvM(mu_init="reference")
    torch.manual_seed(0)
    spread = PointNetPPMvM(mu_init="spread")
    assert not ref.head_mu.weight.any() and not ref.head_mu.bias.any()
    sd_ref, sd_named, sd_spread = ref.state_dict(), named.state_dict(), spread.state_dict()
    assert list(sd_ref) == list(sd_named) == list(sd_spread)
    for k in sd_ref:
        assert torch.equal(sd_ref[k], sd_named[k]), k
        if k != "head_mu.bias":
            assert torch.equal(sd_ref[k], sd_spread[k]), k
    ang = 2.0 * math.pi * torch.arange(4, dtype=torch.float64) / 4
    want = torch.stack((ang.cos(), ang.sin()), dim=1).flatten().float()
    assert torch.equal(sd_spread["head_mu.bias"], want)
    assert not spread.head_mu.weight.any()
    eight = PointNetPPMvM(max_K=8, mu_init="spread").head_mu.bias.detach().view(8, 2).double()
    assert torch.allclose(torch.atan2(eight[:, 1], eight[:, 0]) % (2 * math.pi), 2.0 * math.pi * torch.arange(8, dtype=torch.float64) / 8,
                          atol=1e-6)
    with pytest.raises(ValueError):
        PointNetPPMvM(mu_init="random")


def test_script_defaults(monkeypatch):
    monkeypatch.delenv("PNPP_MVM_LOSS", raising=False)
    import train_multi_peaks_vonMises_KL as T
    args = T._parser().parse_args([])
    assert args.loss == "match" and args.mu_init == "reference"
    assert T._LOSSES["match"] is T._loss and T._loss[1] is T._criterion
    args = T._parser().parse_args(["--loss", "grid-kl", "--mu-init", "spread"])
    assert args.loss == "grid-kl" and args.mu_init == "spread" and T._LOSSES["grid-kl"][1] is T._criterion_grid_kl
    with pytest.raises(SystemExit):
        T._parser().parse_args(["--loss", "other"])


# ---- the C entry points' refusals ----------------------------------------------------------------------------------------------------
P = 8   # any non-null address: nothing is read before the checks


def _plain(h, mu=P, kappa=P, weight=P, vm_gt=P, K_gt=P, B=2, maxK=4, num=360, loss=P, dmu=None, dkappa=None, dweight=None):
    return h.pnpp_mvm_grid_kl(mu, kappa, weight, vm_gt, K_gt, B, maxK, num, loss, dmu, dkappa, dweight, None)


def _headed(h, pi_raw=P, mu_raw=P, kappa_raw=P, vm_gt=P, K_gt=P, B=2, maxK=4, temp=0.7, kappa_max=80.0, num=360, loss=P, dpi=None,
            dmu=None, dkappa=None, mu=None, kappa=None, weight=None):
    return h.pnpp_mvm_head_grid_kl(pi_raw, mu_raw, kappa_raw, vm_gt, K_gt, B, maxK, temp, kappa_max, num, loss, dpi, dmu, dkappa, mu, kappa,
                                   weight, None)


@pytest.mark.parametrize("call,prefix,inputs", [(_plain, b"mvm_grid_kl: ", ("mu", "kappa", "weight")),
                                                (_headed, b"mvm_head_grid_kl: ", ("pi_raw", "mu_raw", "kappa_raw"))])
def test_refusals(h, call, prefix, inputs):
    from pnpp_hip import _lib
    table = [(dict([(name, None)]), b"null pointer") for name in inputs + ("vm_gt", "K_gt", "loss")]
    table += [(dict(B=0), b"B=0"), (dict(B=-4), b"B=-4"), (dict(maxK=0), b"maxK=0"), (dict(maxK=9), b"maxK=9"), (dict(maxK=-1), b"maxK=-1"),
              (dict(num=2), b"num=2"), (dict(num=1026), b"num=1026"), (dict(num=0), b"num=0"), (dict(num=-7), b"num=-7"),
              (dict(dmu=P), b"all three gradient outputs or none"), (dict(dmu=P, dkappa=P), b"all three gradient outputs or none")]
    if call is _headed:
        table += [(dict(mu=P), b"all three head outputs or none"), (dict(temp=0.0), b"temp=0")]
    for kw, words in table:
        assert call(h, **kw) == _lib.PNPP_ERR_ARG, kw
        assert h.pnpp_last_error().startswith(prefix) and words in h.pnpp_last_error(), (kw, h.pnpp_last_error())


def test_header_and_binding(h):
    import os
    import re
    from conftest import ROOT
    from pnpp_hip import _lib, build
    hdr = open(os.path.join(ROOT, "include", "pnpp_hip.h")).read()
    for name in ("pnpp_mvm_grid_kl", "pnpp_mvm_head_grid_kl"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(h, name)
    assert build.SOURCES["mixture_loss_kernels.hip"] == build.SOURCES["loss_kernels.hip"]   # the head form is held bit-equal across them
    assert h.pnpp_abi_version() == 5
