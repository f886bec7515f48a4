"""The mixture KL on the decode grid on the GPU (csrc/mixture_loss_kernels.hip through pnpp_hip.ops) against its float64 restatement
tests/grid_kl_ref.py.

The gate comes from the number formats, not from the kernel: for the loss and for each gradient, elementwise,
    |got - ref| <= 1.2e-7 |ref| + 1e-12 max(1, max |ref|)
one rounding of a float64 value to float32, plus float64 summation order (the construction of the density gate in
tests/test_gpu_decode.py).  No row of a case is left out.  The head form is held BIT-equal to mvm_head -> mvm_grid_kl -> mvm_head's
backward: the same device functions in the same order, built with the same flags."""
import functools
import math

import numpy as np
import pytest
import torch

import grid_kl_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
NAMES = ("loss", "dmu", "dkappa", "dweight")


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Computed once per case, shared by the tests that need it, never written to."""
    out = R.batch(*CASES[name])
    for a in out:
        a.setflags(write=False)
    return out


def _raw_call(mu, kappa, weight, vm_gt, K_gt, num, grads=True):
    """pnpp_mvm_grid_kl itself: (loss, dmu, dkappa, dweight) or (loss,) with null gradient pointers."""
    from pnpp_hip import _lib
    t = [_dev(mu), _dev(kappa), _dev(weight), _dev(vm_gt), _dev(K_gt, torch.int32)]
    B, K = t[0].shape
    out = [torch.full((B,), float("nan")).cuda()] + ([torch.full((B, K), float("nan")).cuda() for _ in range(3)] if grads else [])
    ptr = [o.data_ptr() for o in out] + [None] * (4 - len(out))
    _lib.check(_lib.lib().pnpp_mvm_grid_kl(*[x.data_ptr() for x in t], B, K, num, *ptr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


def _excess(got, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(got.cpu().double().numpy() - ref) - (1.2e-7 * np.abs(ref) + 1e-12 * max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_the_restatement(name):
    mu, kappa, weight, vm_gt, K_gt, num = CASES[name]
    ref = _reference(name)
    assert all(np.isfinite(r).all() and np.abs(r).max() < 1e30 for r in ref), "the case table must stay inside float32"
    got = _raw_call(mu, kappa, weight, vm_gt, K_gt, num)
    worst = {}
    for what, g, r in zip(NAMES, got, ref):
        assert g.shape == r.shape and torch.isfinite(g).all(), what
        worst[what] = float(_excess(g, r).max())
        rel = np.abs(g.cpu().double().numpy() - r) / np.maximum(np.abs(r), 1e-300)
        print(f"  {name} {what}: excess {worst[what]:.2e}, worst relative error where |ref| > 1e-6 max: "
              f"{rel[np.abs(r) > 1e-6 * max(np.abs(r).max(), 1e-300)].max(initial=0.0):.2e}")
    assert all(v <= 0.0 for v in worst.values()), worst
    # a clamped kappa gets exactly zero gradient; a dead row is exactly zero everywhere
    clamped = (np.asarray(kappa) > R.KAPPA_CLAMP)
    assert (got[2].cpu().numpy()[clamped] == 0.0).all()
    dead = ref[0] == 0.0
    assert all((g.cpu().numpy()[dead] == 0.0).all() for g in got)
    # evaluation only (null gradient pointers): the same bits; and again: the same bits
    assert torch.equal(_raw_call(mu, kappa, weight, vm_gt, K_gt, num, grads=False)[0], got[0])
    again = _raw_call(mu, kappa, weight, vm_gt, K_gt, num)
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_case_table_covers_what_it_should():
    seen_k, seen_g, seen_b = set(), set(), set()
    for mu, kappa, weight, vm_gt, K_gt, num in CASES.values():
        seen_k.add(mu.shape[1]), seen_g.add(num - 1), seen_b.add(mu.shape[0])
    assert seen_k >= {1, 2, 3, 4, 8} and seen_g >= {2, 8, 255, 256, 257, 359, 1024} and seen_b >= {1, 3, 65}
    mu, kappa, weight, vm_gt, K_gt, num = CASES["B65-K4-G359"]
    assert set(K_gt.tolist()) == set(range(6))                                     # 0 .. max_K and one above
    assert (weight == 0.0).any() and (vm_gt[:, :, 2] == 0.0).any() and (np.abs(mu) == R.PI32).any()
    assert (np.abs(vm_gt[:, :, 2].sum(1) - 1.0) > 0.1).any()                       # ground-truth weights that do not sum to 1
    assert (mu[:, 0] == mu[:, 1]).any()                                            # coincident components
    for k in R.KAPPAS:
        assert (kappa == k).any() and (vm_gt[:, :, 1] == k).any()


# ---- the head form ------------------------------------------------------------------------------------------------------------------
def _raws(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    pi = torch.randn(B, K, generator=g)
    mr = torch.randn(B, 2 * K, generator=g)
    kr = torch.randn(B, K, generator=g) * 3
    mr[0] = 0.0                                   # the degenerate fallback: mu = 0, no gradient
    if K >= 2:
        mr[1, :2] = 0.0
    kr[:, 0] = torch.linspace(2.0, 120.0, B)      # beyond kappa_max (softplus(x) ~ x): clamped, no gradient
    return pi.cuda(), mr.cuda(), kr.cuda()


@pytest.mark.parametrize("B,K,num", [(1, 1, 360), (3, 2, 9), (5, 3, 360), (65, 4, 360), (7, 8, 258), (3, 4, 1025)])
def test_head_form_equals_the_composition_bit_for_bit(B, K, num):
    from pnpp_hip import ops
    temp, kmax = 0.7, 80.0
    mu0, kappa0, weight0, vm_gt, K_gt = R.rows(B, K, 31 * B + K)
    vm_gt, K_gt = _dev(vm_gt), _dev(K_gt, torch.int32)
    raws = [t.requires_grad_(True) for t in _raws(B, K, 5 * B + K)]
    mu, kappa, weight = ops.mvm_head(*raws, temp, kmax)
    loss = ops.mvm_grid_kl(mu, kappa, weight, vm_gt, K_gt, num)
    want = torch.autograd.grad(loss.sum(), raws)
    fused = [t.detach().clone().requires_grad_(True) for t in raws]
    floss, fmu, fkappa, fweight = ops.mvm_head_grid_kl(*fused, vm_gt, K_gt, temp, kmax, num, outputs=True)
    got = torch.autograd.grad(floss.sum(), fused)
    torch.cuda.synchronize()
    assert not fmu.requires_grad and torch.equal(fmu, mu) and torch.equal(fkappa, kappa) and torch.equal(fweight, weight)
    assert torch.equal(floss, loss)
    for what, a, b in zip(("dpi_raw", "dmu_raw", "dkappa_raw"), got, want):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))
    assert not got[1][0].any() and (got[2][:, 0][raws[2][:, 0] > kmax] == 0.0).all()
    assert torch.equal(ops.mvm_head_grid_kl(*[t.detach() for t in raws], vm_gt, K_gt, temp, kmax, num), loss)   # evaluation only


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
def test_autograd_scales_per_row():
    from pnpp_hip import ops
    name = "B65-K4-G359"
    mu, kappa, weight, vm_gt, K_gt, num = CASES[name]
    B = len(mu)
    base = _raw_call(mu, kappa, weight, vm_gt, K_gt, num)
    gt, kg = _dev(vm_gt), _dev(K_gt, torch.int32)
    leaves = [_dev(a).requires_grad_(True) for a in (mu, kappa, weight)]
    loss = ops.mvm_grid_kl(*leaves, gt, kg, num)
    assert torch.equal(loss, base[0])
    loss.mean().backward()
    for leaf, per_sample in zip(leaves, base[1:]):
        assert torch.equal(leaf.grad, per_sample * torch.full((B, 1), 1.0 / B).cuda())
    g = torch.linspace(-2.0, 3.0, B).cuda()
    for leaf, per_sample, got in zip(leaves, base[1:], torch.autograd.grad((ops.mvm_grid_kl(*leaves, gt, kg, num) * g).sum(), leaves)):
        assert torch.equal(got, per_sample * g[:, None])
    # the head form: the same rule on its raw gradients
    raws = [t.requires_grad_(True) for t in _raws(B, 4, 3)]
    per = torch.autograd.grad(ops.mvm_head_grid_kl(*raws, gt, kg, 0.7, 80.0, num).sum(), raws)
    ops.mvm_head_grid_kl(*raws, gt, kg, 0.7, 80.0, num).mean().backward()
    for r, p in zip(raws, per):
        assert torch.equal(r.grad, p * torch.full((B, 1), 1.0 / B).cuda())
    for p, got in zip(per, torch.autograd.grad((ops.mvm_head_grid_kl(*raws, gt, kg, 0.7, 80.0, num) * g).sum(), raws)):
        assert torch.equal(got, p * g[:, None])


def test_refuses_wrong_shapes():
    from pnpp_hip import ops
    z = lambda *s: torch.zeros(*s).cuda()
    kg = torch.ones(2, dtype=torch.int32).cuda()
    with pytest.raises(ValueError):
        ops.mvm_grid_kl(z(2, 9), z(2, 9), z(2, 9), z(2, 9, 3), kg)               # max_K > 8
    with pytest.raises(ValueError):
        ops.mvm_grid_kl(z(2, 4), z(2, 3), z(2, 4), z(2, 4, 3), kg)
    with pytest.raises(ValueError):
        ops.mvm_grid_kl(z(2, 4), z(2, 4), z(2, 4), z(2, 4, 2), kg)
    with pytest.raises(ValueError):
        ops.mvm_grid_kl(z(2, 4), z(2, 4), z(2, 4), z(2, 4, 3), kg[:1])
    with pytest.raises(ValueError):
        ops.mvm_grid_kl(z(2, 4), z(2, 4), z(2, 4), z(2, 4, 3), kg, num=2)
    with pytest.raises(ValueError):
        ops.mvm_head_grid_kl(z(2, 9), z(2, 18), z(2, 9), z(2, 9, 3), kg, 0.7, 80.0)
    with pytest.raises(ValueError):
        ops.mvm_head_grid_kl(z(2, 4), z(2, 4), z(2, 4), z(2, 4, 3), kg, 0.7, 80.0)   # mu_raw is (B, 2 max_K)


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_forward_and_backward():
    from pnpp_hip import ops
    data = [R.rows(16, 4, s) for s in (201, 202, 203)]
    static = [_dev(a).clone() for a in data[0][:4]] + [_dev(data[0][4], torch.int32).clone()]
    for t in static[:3]:
        t.requires_grad_(True)

    def run():
        loss = ops.mvm_grid_kl(*static, 360)
        return (loss, *torch.autograd.grad(loss.sum(), static[:3]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for d in data[1:]:
        with torch.no_grad():
            for s, a in zip(static[:4], d[:4]):
                s.copy_(_dev(a))
            static[4].copy_(_dev(d[4], torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, _raw_call(*d, 360)):
            assert torch.equal(a, b)


# ---- descent ------------------------------------------------------------------------------------------------------------------------
def test_descent_on_raw_head_parameters():
    """Plain gradient descent, lr 0.1, 40 steps, from pi_raw = kappa_raw = 0 and mu_raw at 2 pi i / 4 - pi + 0.1 towards peaks at 0.3 and
    0.3 - pi: the loss falls at every step (the float64 restatement: 0.7307 -> 0.7036 in steps of about 7e-4)."""
    from pnpp_hip import ops
    K = 4
    gt, kg = _dev(R.descent_gt(K))[None], torch.tensor([2], dtype=torch.int32).cuda()
    raws = [torch.zeros(1, K).cuda(), _dev(R.descent_mu_raw(K))[None].clone(), torch.zeros(1, K).cuda()]
    want, losses = R.descent(), []
    for _ in range(40):
        leaves = [r.detach().requires_grad_(True) for r in raws]
        loss = ops.mvm_head_grid_kl(*leaves, gt, kg, 0.7, 80.0)
        grads = torch.autograd.grad(loss.sum(), leaves)
        losses.append(float(loss.detach()))
        raws = [r - 0.1 * g for r, g in zip(leaves, grads)]
    print(f"  descent: {losses[0]:.6f} -> {losses[-1]:.6f}; restatement {want[0]:.6f} -> {want[39]:.6f}")
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert abs(losses[0] - want[0]) < 1e-6 and abs(losses[-1] - want[39]) < 1e-4


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_model_defect_and_remedy_side_by_side():
    from models.pointnet_pp_mvM import PointNetPPMvM
    from pnpp_hip import ops
    B, N = 4, 128
    g = torch.Generator().manual_seed(4)
    xyz = torch.randn(B, N, 3, generator=g).cuda()
    vm_gt = torch.zeros(B, 4, 3)
    vm_gt[:, 0] = torch.tensor([0.3, 8.0, 0.5])
    vm_gt[:, 1] = torch.tensor([0.3 - math.pi, 8.0, 0.5])
    vm_gt, K_gt = vm_gt.cuda(), torch.full((B,), 2, dtype=torch.int32).cuda()

    torch.manual_seed(0)
    model = PointNetPPMvM(mu_init="spread", sampler="device").cuda().train()
    loss = model.grid_kl(xyz, vm_gt, K_gt)
    assert loss.shape == (B,) and torch.isfinite(loss).all()
    loss.mean().backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert model.head_mu.weight.grad.any()                                         # the remedy: mu learns

    torch.manual_seed(0)
    ref = PointNetPPMvM(mu_init="reference", sampler="device").cuda().train()
    mu, kappa, weight = ref(xyz)
    ops.match_loss(mu, kappa, weight, vm_gt, K_gt).mean().backward()
    assert not ref.head_mu.weight.grad.any() and not ref.head_mu.bias.grad.any()   # the defect: mu gets no gradient


def test_losses_wrapper():
    import losses
    name = "B3-K4-G359"
    mu, kappa, weight, vm_gt, K_gt, num = CASES[name]
    got = losses.mixture_grid_kl((_dev(mu), _dev(kappa), _dev(weight)), _dev(vm_gt), _dev(K_gt, torch.int32), num)
    assert torch.equal(got, _raw_call(mu, kappa, weight, vm_gt, K_gt, num)[0])


def test_training_script_with_grid_kl(tmp_path, monkeypatch):
    """--loss grid-kl --mu-init spread through the multi-peak script's own loop: the same result files under the same names, finite
    losses for train, val and test, and a mu head that has moved.  (The figures are test_gpu_train.py's business: not drawn here.)"""
    import train_multi_peaks_vonMises_KL as t
    from models.pointnet_pp_mvM import PointNetPPMvM
    for name, value in (("RES", tmp_path), ("FIGS", tmp_path / "figs"), ("EPOCHS", 2), ("BATCH", 16), ("NUM_POINTS", 256)):
        monkeypatch.setattr(t, name, value)
    for name in ("plot_curve", "plot_pair"):
        monkeypatch.setattr(t, name, lambda *a, **k: None)
    hist, test_kl = t.main(["--synthetic", "64", "--sampler", "device", "--loss", "grid-kl", "--mu-init", "spread"])
    assert len(hist["total"]["train"]) == 2 and all(math.isfinite(v) and v > 0.0 for v in hist["total"]["train"] + hist["total"]["val"])
    assert math.isfinite(test_kl) and test_kl > 0.0
    assert {"mvM_best.pth", "results.txt"} <= {p.name for p in tmp_path.iterdir()}
    sd = torch.load(tmp_path / "mvM_best.pth")
    PointNetPPMvM().load_state_dict(sd)                                             # the reference's keys
    assert sd["head_mu.weight"].any()
