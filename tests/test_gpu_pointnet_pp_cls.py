"""The PointNet++ classifier port on the GPU (models/pointnet_pp_cls.py, csrc/cls_loss_kernels.hip, the wide instantiation of
csrc/sa_infer_kernels.hip, pnpp_hip.inference.ClsPredictor).

Gates are those of the tests each part belongs with: the loss operators as tests/test_gpu_head_loss.py gates soft_ce (rtol 1e-5,
atol 1e-6 against float64); a bare level as tests/test_gpu_sa.py (3e-5 of the tensor's max-abs for outputs and gradients, 1e-5 for
running statistics); the fused level launch and the Predictor as tests/test_gpu_inference.py's _compare (1e-4 * max(1, max|ref|));
the model against the reference's capture as tests/test_gpu_pointnet.py (its _check_grads / _check_after are imported).
The levels across the dispatcher's kernel bands, routed float64 at 1e-5 with the kernels asserted: tests/test_gpu_cls_bands.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import has_gpu, relmax

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an AMD GPU")]

EPS = 1e-5


# ------------------------------------------------------------------------------------------------ (a) log_softmax / nll_loss
@pytest.mark.parametrize("M,Cc", [(1, 2), (5, 40), (33, 1000)])
def test_log_softmax_nll_loss_vs_float64(M, Cc):
    from pnpp_hip import ops
    g = torch.Generator().manual_seed(M * 1000 + Cc)
    x = 3.0 * torch.randn(M, Cc, generator=g)
    x[M // 2, Cc // 3] = x[M // 2].max() + 80.0          # one logit 80 above the rest of its row
    t = torch.randint(0, Cc, (M,), generator=g)
    t[M // 2] = (Cc // 3 + 1) % Cc                       # ... and the target on a class whose probability is ~e^-80
    up = torch.randn(M, Cc, generator=g)                 # an upstream gradient for log_softmax on its own

    xd = x.double().requires_grad_(True)
    yd = torch.log_softmax(xd, 1)
    ld = torch.nn.functional.nll_loss(yd, t)
    gx_loss, = torch.autograd.grad(ld, xd, retain_graph=True)
    gx_up, = torch.autograd.grad((yd * up.double()).sum(), xd)

    xg = x.cuda().requires_grad_(True)
    y = ops.log_softmax(xg)
    loss = ops.nll_loss(y, t.cuda())
    hx_loss, = torch.autograd.grad(loss, xg, retain_graph=True)
    hx_up, = torch.autograd.grad((y * up.cuda()).sum(), xg)
    assert y.shape == (M, Cc) and loss.shape == ()
    for what, got, ref in (("log_softmax", y, yd), ("nll_loss", loss, ld), ("d loss / dx", hx_loss, gx_loss), ("d (y . up) / dx", hx_up, gx_up)):
        got, ref = got.detach().cpu().double().numpy(), ref.detach().numpy()
        print(f"  {M} x {Cc} {what}: max |err| {np.abs(got - ref).max():.3e}")
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-6), what
    # int32 targets are taken as they are; two runs agree bit for bit
    again = ops.nll_loss(ops.log_softmax(xg), t.cuda().to(torch.int32))
    assert torch.equal(again, loss)


def test_nll_loss_target_out_of_range_is_an_error_not_an_abort():
    from pnpp_hip import ops
    logp = ops.log_softmax(torch.randn(6, 10, device="cuda"))
    for bad in (10, -1, -100):
        t = torch.tensor([0, 3, bad, 9, 1, 2], device="cuda")
        with pytest.raises(RuntimeError, match=r"1 of 6 targets lie outside \[0, 10\)"):
            ops.nll_loss(logp, t)
    t = torch.tensor([0, 3, 10, 9, 1, 2], device="cuda")
    ok = torch.tensor([0, 3, 9, 1, 2], device="cuda")
    loose = ops.nll_loss(logp, t, check=False)            # unchecked: the row adds nothing, the mean is still over M
    keep = torch.tensor([0, 1, 3, 4, 5], device="cuda")
    assert torch.allclose(loose * 6, ops.nll_loss(logp[keep], ok) * 5, rtol=1e-6)
    assert torch.isfinite(ops.nll_loss(logp, torch.zeros(6, dtype=torch.long, device="cuda")))   # the process is alive and well


# ------------------------------------------------------------------------------------------------ float64 restatement of a level
def _randomise(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                n = m.num_features
                m.weight.copy_(0.5 + torch.rand(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(n, generator=g))
                m.running_var.copy_(torch.exp(math.log(0.05) + torch.rand(n, generator=g) * (math.log(2.0) - math.log(0.05))))
    return mod


def _params64(level, device):
    """per layer (W (C, Cin), b, gamma, beta, running_mean, running_var) in float64; the first four as leaves"""
    out = []
    for conv, bn in zip(level.mlp_convs, level.mlp_bns):
        leaf = [t.detach().to(device).double().requires_grad_(True) for t in (conv.weight.flatten(1), conv.bias, bn.weight, bn.bias)]
        out.append(leaf + [bn.running_mean.detach().to(device).double(), bn.running_var.detach().to(device).double()])
    return out


def _level64(xyz, pts, centre, nbr, params, training, fold=False):
    """PointNet++Demo.py:107-127 / :159-169 in float64 on given indices: gather (coordinates relative to the centre, then the
    features), len(params) x (1x1 conv, BatchNorm, ReLU), max over the neighbourhood.  nbr None: the whole cloud, absolute
    coordinates.  fold: the BatchNorm as the affine map of its running statistics folded into the convolution (W', b').
    -> (B, S, C), [(batch mean, unbiased batch variance) per layer]"""
    B = xyz.shape[0]
    if nbr is None:
        rows = (xyz if pts is None else torch.cat([xyz, pts], -1))[:, None]
    else:
        b3 = torch.arange(B, device=xyz.device)[:, None, None]
        rel = xyz[b3, nbr] - xyz[b3[:, :, 0], centre][:, :, None]
        rows = rel if pts is None else torch.cat([rel, pts[b3, nbr]], -1)
    h, stats = rows, []
    for W, b, gamma, beta, rm, rv in params:
        if fold:
            a = gamma / torch.sqrt(rv + EPS)
            h = torch.relu(h @ (a[:, None] * W).t() + ((b - rm) * a + beta))
            continue
        z = h @ W.t() + b
        if training:
            n = z.numel() // z.shape[-1]
            mu, var = z.mean((0, 1, 2)), z.var((0, 1, 2), unbiased=False)
            stats.append((mu.detach(), var.detach() * n / (n - 1)))
        else:
            mu, var = rm, rv
        h = torch.relu((z - mu) / torch.sqrt(var + EPS) * gamma + beta)
    return h.max(2).values, stats


# ------------------------------------------------------------------------------------------------ (b) a bare level with D = 3
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bare_level_with_three_feature_channels(training):
    from pnpp_hip import ops
    from models.pointnet_pp_cls import SimpleSetAbstraction
    B, N, S, K, D = 3, 70, 5, 32, 3
    torch.manual_seed(11)
    sa = _randomise(SimpleSetAbstraction(S, 0.45, K, D, [64, 64, 128]), 12)
    g = torch.Generator().manual_seed(13)
    xyz, pts = torch.rand(B, N, 3, generator=g), torch.rand(B, N, D, generator=g)
    start = torch.randint(0, N, (B,), generator=g)
    gy = torch.randn(B, S, 128, generator=g)
    P = _params64(sa, "cpu")
    rm0 = [bn.running_mean.clone() for bn in sa.mlp_bns]
    sa = sa.cuda().train(training)

    xg, pg = xyz.cuda(), pts.cuda()
    centre = ops.farthest_point_sample(xg, S, start)
    nbr = ops.ball_query(0.45, K, xg, ops.index_points(xg, centre))
    counts = [(n[1:] != n[0]).sum().item() + 1 for n in nbr.cpu().reshape(-1, K)]
    assert min(counts) < K, "the radius should leave some neighbourhoods padded"
    new_xyz, y = sa.rows(xg, pg, start)
    y.backward(gy.cuda())
    torch.cuda.synchronize()

    y64, stats = _level64(xyz.double(), pts.double(), centre.cpu().long(), nbr.cpu().long(), P, training)
    (y64 * gy.double()).sum().backward()
    assert torch.equal(new_xyz.cpu(), xyz[torch.arange(B)[:, None], centre.cpu().long()])
    e = relmax(y, y64)
    print(f"  D=3 level ({'train' if training else 'eval'}): out relmax {e:.3e}")
    assert e < 3e-5
    for l, (conv, bn) in enumerate(zip(sa.mlp_convs, sa.mlp_bns)):
        for name, p, ref in (("weight", conv.weight, P[l][0].grad), ("bias", conv.bias, P[l][1].grad), ("gamma", bn.weight, P[l][2].grad),
                             ("beta", bn.bias, P[l][3].grad)):
            if training and name == "bias":   # cancels in a train-mode BatchNorm
                assert float(p.grad.abs().max()) == 0.0 and float(ref.abs().max()) < 1e-9, (l, name)
                continue
            e = relmax(p.grad.flatten(1) if name == "weight" else p.grad, ref)
            print(f"    layer {l} d{name}: {e:.3e}")
            assert e < 3e-5, (l, name)
        if training:
            mu, var = stats[l]
            assert relmax(bn.running_mean, 0.9 * rm0[l].double() + 0.1 * mu) < 1e-5
            assert relmax(bn.running_var, 0.9 * P[l][5] + 0.1 * var) < 1e-5
            assert int(bn.num_batches_tracked) == 1
        else:
            assert torch.equal(bn.running_mean.cpu(), rm0[l]) and int(bn.num_batches_tracked) == 0
    # the reference's channels-first interface of the module is the same computation
    torch.manual_seed(5)
    with torch.no_grad():
        sa.eval()
        a_xyz, a_pts = sa(xg.transpose(1, 2), pg.transpose(1, 2), start)
        b_xyz, b_pts = sa.rows(xg, pg, start)
    assert torch.equal(a_xyz, b_xyz.transpose(1, 2)) and torch.equal(a_pts, b_pts.transpose(1, 2))


# ------------------------------------------------------------------------------------------------ (c) pnpp_sa_infer at the new sizes
GUARD_FILL = -12345.678


def _sa_infer(level, xyz, pts, centre, nbr, K, group_all, guard=0, idx_out=None):
    """fold + one pnpp_sa_infer launch on a level's own tensors -> (new_xyz, out), both pre-filled with NaN.
    guard: that many more groups, filled with GUARD_FILL, lie behind the real ones in both buffers and are returned as a third
    element (guard rows of new_xyz, guard rows of out).  nbr None with idx_out (B, S, K) int32: the level searches its own
    neighbours and writes them there."""
    from pnpp_hip import _lib as L, ops
    lib = L.lib()
    B, N, _ = xyz.shape
    S = 1 if group_all else centre.shape[1]
    ch = [c.weight.shape[0] for c in level.mlp_convs]
    d = ops._sa_desc(B, N, S, K, 0 if pts is None else pts.shape[2], ch, group_all, False, EPS, 0.1)
    assert lib.pnpp_sa_infer_supported(C.byref(d)) == 1, lib.pnpp_last_error()
    blob = torch.empty(lib.pnpp_sa_infer_weights_bytes(C.byref(d)), dtype=torch.uint8, device="cuda")
    a = L.SaFwdArgs()
    keep = []
    for field, ts in (("conv_w", [c.weight for c in level.mlp_convs]), ("conv_b", [c.bias for c in level.mlp_convs]),
                      ("bn_w", [b.weight for b in level.mlp_bns]), ("bn_b", [b.bias for b in level.mlp_bns]),
                      ("bn_rm", [b.running_mean for b in level.mlp_bns]), ("bn_rv", [b.running_var for b in level.mlp_bns])):
        ts = [t.detach().contiguous() for t in ts]
        keep += ts
        setattr(a, field, ops._ptr_array(ts))
    L.check(lib.pnpp_sa_infer_fold(C.byref(d), C.byref(a), blob.data_ptr(), ops._stream()))
    ia = L.SaInferArgs()
    ia.xyz, ia.points, ia.weights = xyz.data_ptr(), ops._p(pts), blob.data_ptr()
    if not group_all:
        ia.centre_idx, ia.neighbour_idx, ia.idx_out = centre.data_ptr(), ops._p(nbr), ops._p(idx_out)
    new_xyz = torch.full((B * S + guard, 3), float("nan"), device="cuda")
    out = torch.full((B * S + guard, ch[-1]), float("nan"), device="cuda")
    new_xyz[B * S:], out[B * S:] = GUARD_FILL, GUARD_FILL
    ia.new_xyz, ia.out = new_xyz.data_ptr(), out.data_ptr()
    L.check(lib.pnpp_sa_infer(C.byref(d), C.byref(ia), ops._stream()))
    torch.cuda.synchronize()
    res = new_xyz[:B * S].view(B, S, 3), out[:B * S].view(B, S, ch[-1])
    return res + ((new_xyz[B * S:], out[B * S:]),) if guard else res


WIDE = {
    "K64-15-groups": dict(B=3, N=200, S=5, K=64, D=128, ch=[128, 128, 256]),
    "K96-D0": dict(B=2, N=150, S=7, K=96, D=0, ch=[64, 64, 128]),
    "group_all-128-split": dict(B=3, N=128, S=1, K=128, D=256, ch=[256, 512, 1024], group_all=True),
    "group_all-128-B300": dict(B=300, N=128, S=1, K=128, D=256, ch=[256, 512, 1024], group_all=True),
    "K256": dict(B=2, N=400, S=3, K=256, D=0, ch=[64, 64, 128]),
    "K64-padded": dict(B=3, N=200, S=5, K=64, D=128, ch=[128, 128, 256], radius=0.5),
}


@pytest.mark.parametrize("case", list(WIDE))
def test_sa_infer_wide_neighbourhoods(case):
    from pnpp_hip import ops
    from models.pointnet_pp_cls import SimpleSetAbstraction, SimpleSetAbstractionGroupAll
    c = dict(WIDE[case])
    B, N, S, K, D, ch, ga, radius = c["B"], c["N"], c["S"], c["K"], c["D"], c["ch"], c.get("group_all", False), c.get("radius")
    torch.manual_seed(21)
    level = SimpleSetAbstractionGroupAll(D, ch) if ga else SimpleSetAbstraction(S, radius or 1.0, K, D, ch)
    level = _randomise(level, 22).cuda().eval()
    g = torch.Generator().manual_seed(23)
    xyz = torch.rand(B, N, 3, generator=g).cuda()
    pts = torch.randn(B, N, D, generator=g).cuda() if D else None
    centre = nbr = None
    if not ga:
        centre = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)]).to(torch.int32).cuda()
        if radius is None:
            nbr = torch.randint(0, N, (B, S, K), generator=g).to(torch.int32).cuda()
        else:   # as the radius query pads them: short neighbourhoods repeat their first member
            nbr = ops.ball_query(radius, K, xyz, ops.index_points(xyz, centre))
            short = (nbr[..., 1:] == nbr[..., :1]).any(-1)
            assert bool(short.any()) and not bool(short.all())
    new_xyz, out = _sa_infer(level, xyz, pts, centre, nbr, K, ga)
    with torch.no_grad():   # the float64 evaluation of the same folded level, on the device
        ref, _ = _level64(xyz.double(), None if pts is None else pts.double(), None if ga else centre.long(), None if ga else nbr.long(),
                          _params64(level, "cuda"), False, fold=True)
    d = float((out.double() - ref).abs().max())
    gate = 1e-4 * max(1.0, float(ref.abs().max()))
    print(f"  {case}: |fused - float64| = {d:.3e} (gate {gate:.1e}, max|ref| {float(ref.abs().max()):.2f})")
    assert not torch.isnan(out).any() and d <= gate
    if ga:
        assert float(new_xyz.abs().max()) == 0.0
    else:
        assert torch.equal(new_xyz, xyz[torch.arange(B, device="cuda")[:, None], centre.long()])
    # the level the library's differentiable eval path computes, for the record
    with torch.no_grad():
        _, ev = ops.set_abstraction(xyz, pts, centre, K, ga, False, level.mlp_convs, level.mlp_bns, neighbour_idx=nbr)
    print(f"  {case}: |fused - eval path| = {float((out - ev).abs().max()):.3e}")


# ------------------------------------------------------------------------------------------------ (d) the model against the fixture
@pytest.fixture(scope="module")
def fixture(golden):
    return golden("pointnet_pp_cls.npz")


def _fixture_model(g):
    from models import PointNetPlusPlusCls
    torch.manual_seed(int(g["cls.seed"]))
    return PointNetPlusPlusCls(num_classes=40).cuda()


def _fixture_inputs(g):
    x = torch.from_numpy(g["cls.x"]).cuda()
    start = tuple(torch.from_numpy(g[f"cls.start{i}"]).cuda() for i in (1, 2))
    return x, start


def test_indices_bit_exact_against_the_reference(fixture):
    from pnpp_hip import ops
    g = fixture
    x, start = _fixture_inputs(g)
    xyz = x[:, :3].transpose(1, 2).contiguous()
    for i, (npoint, radius, nsample) in enumerate(((512, 0.2, 32), (128, 0.4, 64)), 1):
        fps = ops.farthest_point_sample(xyz, npoint, start[i - 1])
        assert np.array_equal(fps.cpu().numpy(), g[f"cls.fps{i}"].astype(np.int32)), f"level {i} centres"
        new_xyz = ops.index_points(xyz, fps)
        nbr = ops.ball_query(radius, nsample, xyz, new_xyz)
        assert np.array_equal(nbr.cpu().numpy(), g[f"cls.nbr{i}"].astype(np.int32)), f"level {i} neighbours"
        xyz = new_xyz


def test_model_vs_reference_capture(fixture):
    from test_gpu_pointnet import _check_after, _check_grads
    from models import get_loss
    g = fixture
    m = _fixture_model(g).train()
    x, start = _fixture_inputs(g)
    masks = tuple(torch.from_numpy(g[f"cls.mask{i}"]).cuda() for i in (1, 2))
    target = torch.from_numpy(g["cls.target"]).cuda()
    logp = m(x, start=start, drop_masks=masks)
    loss = get_loss()(logp, target)
    loss.backward()
    e = np.abs(logp.detach().cpu().double().numpy() - g["cls.logp"]).max()
    print(f"\n[pointnet++ cls] loss {float(loss.detach()):.7f} ref {float(g['cls.loss']):.7f}; max |logp err| {e:.3e}")
    assert logp.shape == (8, 40) and e < 2e-5
    assert abs(float(loss.detach()) - float(g["cls.loss"])) <= 1e-5 * max(1.0, abs(float(g["cls.loss"])))
    worst = _check_grads(g, "cls", m)
    _check_after(g, "cls", m)
    m.eval()
    with torch.no_grad():
        ev = m(x, start=start)
    ee = np.abs(ev.cpu().double().numpy() - g["cls.eval_logp"]).max()
    print(f"[pointnet++ cls] worst sampled grad err {worst:.2e}; eval-mode max |logp err| {ee:.3e}")
    assert ee < 5e-5


def test_reference_draws_one_start_per_level(fixture):
    """without `start` the model draws as PointNet++Demo.py:20 does: torch.randint(0, N, (B,)) on the host generator, sa1 then sa2"""
    g = fixture
    m = _fixture_model(g).eval()
    x, _ = _fixture_inputs(g)
    with torch.no_grad():
        torch.manual_seed(77)
        a = m(x)
        torch.manual_seed(77)
        s1, s2 = torch.randint(0, 1024, (8,)), torch.randint(0, 512, (8,))
        b = m(x, start=(s1, s2))
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ (e) Predictor
def _gate(got, ref, what):
    d = float((got.double() - ref.double()).abs().max())
    gate = 1e-4 * max(1.0, float(ref.abs().max()))
    print(f"  {what}: {d:.3e} (gate {gate:.1e})")
    assert got.shape == ref.shape and got.dtype == ref.dtype and not got.requires_grad and d <= gate, what


def test_predictor_equals_eval_and_refreshes(fixture):
    from pnpp_hip.inference import ClsPredictor, Predictor
    from models import get_loss
    g = fixture
    m = _randomise(_fixture_model(g), 31).eval()
    x, start = _fixture_inputs(g)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    p = Predictor(m)
    assert isinstance(p, ClsPredictor)
    assert p.plan == {k: "fused" for k in ("sa1", "sa2", "sa3", "fc1", "fc2", "fc3")}
    with torch.no_grad():
        ev = m(x, start=start)
    first = p(x, start=start)
    assert p.last_plan == p.plan
    _gate(first, ev, "predictor vs model.eval()")
    assert all(torch.equal(v, state[k]) for k, v in m.state_dict().items()), "a Predictor does not write to its model"
    assert p.persistent_bytes() > 0
    # the same host seed -> the same draws -> the same bits, and the same draws as the model's
    torch.manual_seed(9)
    a = p(x).clone()
    torch.manual_seed(9)
    b = p(x)
    torch.manual_seed(9)
    with torch.no_grad():
        c = m(x)
    assert torch.equal(a, b)
    _gate(a, c, "predictor vs model.eval(), own draws")
    # a snapshot until refresh()
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    get_loss()(m(x, start=start), torch.from_numpy(g["cls.target"]).cuda()).backward()
    opt.step()
    m.eval()
    assert torch.equal(p(x, start=start), first), "a Predictor is a snapshot"
    with torch.no_grad():
        now = m(x, start=start)
    assert float((now - first).abs().max()) > 1e-6, "the training step did not move the model"
    p.refresh()
    _gate(p(x, start=start), now, "after refresh()")


def test_predictor_call_that_a_level_refuses_runs_the_eval_path(fixture):
    """sa2.npoint changed after construction hands sa3 100 rows per cloud, which is no multiple of 32"""
    from pnpp_hip.inference import Predictor
    g = fixture
    m = _randomise(_fixture_model(g), 32).eval()
    x, start = _fixture_inputs(g)
    p = Predictor(m)
    m.sa2.npoint = 100
    got = p(x, start=start)
    with torch.no_grad():
        ev = m(x, start=start)
    assert p.plan["sa3"] == "fused" and p.last_plan["sa3"] == "eval-path" and p.last_plan["sa2"] == "fused"
    _gate(got, ev, "sa3 on the eval path")
