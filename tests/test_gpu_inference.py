"""Forward-only inference path (pnpp_hip.inference.Predictor, csrc/sa_infer_kernels.hip) against the float64 oracle's eval-mode
forward and against the library's existing eval path.  Gates: levels and backbone features relmax <= 1e-5 of the tensor's max-abs
(the G2 gate of tests/test_gpu_levels_routed.py); whole-model outputs 1e-4 * max(1, max|ref|) (tests/test_gpu_fullsize.py's eval
gate); folded parameters <= 1 ulp of the float64 formula rounded to float32.  The forward value is continuous in its inputs, so no
decision of the HIP path is injected into the oracle -- only the centres (and, for radius grouping, the neighbour lists)."""
import ctypes
import math

import pytest
import torch

from conftest import has_gpu, relmax

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an AMD GPU")]

G2 = 1e-5


def _randomise(model, seed):
    """BatchNorm affine parameters and running statistics off their initial values; running_var log-uniform in [0.05, 2], and in
    [5e-4, 2] for sa1's layer 0, which really shows 5e-4 after training (a variance that small in every layer multiplies the
    activations by ~45 per layer and saturates every output map)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                n = m.num_features
                m.weight.copy_(0.5 + torch.rand(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(n, generator=g))
                lo = 5e-4 if m is model.sa1.bns[0] else 0.05
                m.running_var.copy_(torch.exp(math.log(lo) + torch.rand(n, generator=g) * (math.log(2.0) - math.log(lo))))
        model.sa1.bns[0].running_var[0] = 5e-4
    return model


def _state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _model(cls, seed=3, **kw):
    torch.manual_seed(seed)
    m = _randomise(cls(**kw), seed + 100)
    return m.cuda().eval(), _state(m)


def _gate_eval(got, ref, what):
    ref = ref.detach().double()
    d = float((got.detach().cpu().double().reshape(ref.shape) - ref).abs().max())
    gate = 1e-4 * max(1.0, float(ref.abs().max()))
    print(f"  {what}: |predictor - float64| = {d:.3e} (gate {gate:.1e})")
    assert d <= gate, what
    return d


def test_fold_matches_float64_formula(oracle):
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    model, state = _model(PointNetPPVonMises)
    p = Predictor(model)
    torch.cuda.synchronize()
    assert p.plan == {"sa1": "fused", "sa2": "fused", "sa3": "fused", "fc1": "fused", "fc2": "fused"}

    def formula(w, b, pre):
        g, be, rm, rv = (state[f"{pre}.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var"))
        a = g / torch.sqrt(rv + 1e-5)
        w = w.double().reshape(w.shape[0], -1)
        return (a[:, None] * w).float(), ((b.double() - rm) * a + be).float()

    def ulps(got, ref):
        got, ref = got.cpu(), ref.cpu()
        spacing = torch.maximum(torch.abs(torch.nextafter(ref, torch.full_like(ref, float("inf"))) - ref),
                                torch.abs(ref - torch.nextafter(ref, torch.full_like(ref, float("-inf")))))
        return float(((got.double() - ref.double()).abs() / spacing.double()).max())

    worst = 0.0
    for s in ("sa1", "sa2", "sa3"):
        for l in range(3):
            w, b, pad = p.folded_layer(s, l)
            wr, br = formula(state[f"{s}.convs.{l}.weight"], state[f"{s}.convs.{l}.bias"], f"{s}.bns.{l}")
            uw, ub = ulps(w, wr), ulps(b, br)
            print(f"  {s} layer {l}: W' {uw:.2f} ulp, b' {ub:.2f} ulp")
            assert uw <= 1.0 and ub <= 1.0, (s, l)
            assert pad.numel() == 0 or float(pad.abs().max()) == 0.0
            worst = max(worst, uw, ub)
    for i in (1, 2):
        f = p._heads[f"fc{i}"]
        wr, br = formula(state[f"fc{i}.weight"], state[f"fc{i}.bias"], f"bn{i}")
        assert ulps(f.weight, wr) <= 1.0 and ulps(f.bias, br) <= 1.0, i


def test_level_parity_g2(oracle):
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    B, N = 32, 1024
    model, state = _model(PointNetPPVonMises)
    P = oracle.cast_params(state, torch.float64, requires_grad=False)
    p = Predictor(model)
    xyz, _, _, _ = oracle.synthetic_clouds(B, N, seed=1234)
    torch.manual_seed(7)
    c1, c2 = oracle.replay_centres(B)
    with torch.no_grad():
        # every level gets the float64 oracle's output of the level above (rounded to float32) as its input, on all three paths
        x1, f1, _ = oracle.sa_forward(xyz, None, P, "sa1", c1, 32, False, training=False)
        x2, f2, _ = oracle.sa_forward(x1, f1, P, "sa2", c2, 32, False, training=False)
        _, f3, _ = oracle.sa_forward(x2, f2, P, "sa3", None, None, True, training=False)
        cases = [(0, model.sa1, xyz, None, c1, f1), (1, model.sa2, x1, f1.float(), c2, f2), (2, model.sa3, x2, f2.float(), None, f3)]
        for i, sa, x, pts, c, ref in cases:
            xg, pg, cg = x.cuda(), None if pts is None else pts.cuda(), None if c is None else c.cuda()
            nx_e, out_e, nbr_e = ops.set_abstraction(xg, pg, cg, sa.nsample, sa.group_all, False, sa.convs, sa.bns, return_neighbours=True)
            nx_f, out_f = p._level(i, xg, pg, cg)
            torch.cuda.synchronize()
            ef, ee = relmax(out_f, ref), relmax(out_e, ref)
            print(f"  sa{i + 1}: fused {ef:.3e}   existing eval path {ee:.3e}   (relmax vs float64, gate {G2:.0e})")
            assert ef <= G2, f"sa{i + 1}"
            assert torch.equal(nx_f, nx_e), f"sa{i + 1} new_xyz"
            assert out_f.shape == out_e.shape and not out_f.requires_grad
            if not sa.group_all:
                nbr_f = p._buf(f"sa{i + 1}.idx", (B, sa.npoint, sa.nsample), torch.int32)
                assert torch.equal(nbr_f.sort(-1).values, nbr_e.to(torch.int32).sort(-1).values), f"sa{i + 1} neighbours"


def _features_case(oracle, model, state, xyz, centres, cfg, routing=None, what=""):
    """the Predictor's backbone features (B, 1024) against oracle.backbone_forward in float64, eval mode"""
    from pnpp_hip.inference import Predictor
    p = Predictor(model)
    P = oracle.cast_params(state, torch.float64, requires_grad=False)
    with torch.no_grad():
        l2_xyz, l2_pts = p._levels12(xyz.cuda(), None if centres is None else [c.cuda() for c in centres])
        feat = p._level(2, l2_xyz, l2_pts)[1].reshape(xyz.shape[0], -1).clone()
        torch.cuda.synchronize()
        ref = oracle.backbone_forward(xyz, P, centres, training=False, cfg=cfg, routing=routing)
    e = relmax(feat, ref)
    print(f"  {what}: backbone features relmax {e:.3e} (gate {G2:.0e}); plan {p.plan}")
    assert e <= G2, what
    return p, feat


@pytest.mark.parametrize("B,N,S1,S2", [(1, 1024, 128, 32), (36, 1024, 77, 32), (16, 10000, 128, 32), (3, 32, 32, 32)],
                         ids=["B1", "B36", "N10000", "N-equals-K"])
def test_shape_bands(oracle, B, N, S1, S2):
    """B = 1; B = 36 with 77 centres per cloud; long clouds; N == K.
    The B = 36 case has FULL tiles at every level, and no B can change that inside a model the kernel takes whole: a tile holds
    64 / K groups, B * S groups are odd only for odd S, sa2 must hand sa3 16 or 32 rows per cloud (an even S), and sa3's tile is
    exactly one cloud (TM = 32 >= K).  Partial last tiles are what test_partial_last_tile_every_level builds: an odd group count
    at sa1 (S = 33 with K = 32 and with K = 16) and at sa2 on its own (S = 31)."""
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    model, state = _model(PointNetPPVonMises)
    model.sa1.npoint = S1
    xyz, _, _, _ = oracle.synthetic_clouds(B, N, seed=99)
    torch.manual_seed(5)
    centres = oracle.replay_centres(B, sizes=((N, S1), (S1, S2)))
    _features_case(oracle, model, state, xyz, centres, ((S1, 32), (S2, 32)), what=f"B={B} N={N} S1={S1}")


def test_partial_last_tile_every_level(oracle):
    """odd group counts at sa1 and sa2 (two groups per 64-row tile) and an odd cloud count at sa3"""
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    model, state = _model(PointNetPPVonMises)
    B, N, S1, S2 = 3, 512, 33, 32
    model.sa1.npoint = S1
    model.sa2.npoint = S2
    xyz, _, _, _ = oracle.synthetic_clouds(B, N, seed=11)
    torch.manual_seed(6)
    centres = oracle.replay_centres(B, sizes=((N, S1), (S1, S2)))
    assert (B * S1) % 2 == 1
    _features_case(oracle, model, state, xyz, centres, ((S1, 32), (S2, 32)), what="odd group counts")
    # K = 16: four groups per 64-row tile, 5 * 33 = 165 groups -> a last tile with one group
    B = 5
    model2, state2 = _model(PointNetPPVonMises)
    model2.sa1.nsample = 16
    model2.sa1.npoint = 33
    xyz, _, _, _ = oracle.synthetic_clouds(B, N, seed=12)
    centres = oracle.replay_centres(B, sizes=((N, 33), (33, 32)))
    p2, _ = _features_case(oracle, model2, state2, xyz, centres, ((33, 16), (32, 32)), what="K=16, 165 groups")
    # sa2 alone with 31 centres per cloud: 3 * 31 = 93 groups, an odd count (inside a model sa3 would then pool 31 rows: eval-path)
    B = 3
    P = oracle.cast_params(state2, torch.float64, requires_grad=False)
    g = torch.Generator().manual_seed(13)
    x1 = oracle.synthetic_clouds(B, 128, seed=14)[0]
    f1 = torch.randn(B, 128, 128, generator=g)
    c2 = torch.stack([torch.randperm(128, generator=g)[:31] for _ in range(B)])
    model2.sa2.npoint = 31
    with torch.no_grad():
        nx, out = p2._level(1, x1.cuda(), f1.cuda(), c2.cuda())
        torch.cuda.synchronize()
        rx, ref, _ = oracle.sa_forward(x1, f1.double(), P, "sa2", c2, 32, False, training=False)
    e = relmax(out, ref)
    print(f"  sa2 alone, 93 groups: relmax {e:.3e}")
    assert e <= G2 and torch.equal(nx.cpu(), rx)


def test_fps_sampler(oracle):
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    B, N = 4, 1024
    model, state = _model(PointNetPPVonMises, sampler="fps")
    xyz, _, _, _ = oracle.synthetic_clouds(B, N, seed=21)
    xg = xyz.cuda()
    p = Predictor(model)
    with torch.no_grad():
        torch.manual_seed(31)
        got = p(xg)
        torch.manual_seed(31)   # the same start draws -> the same farthest-point centres
        c1 = ops.farthest_point_sample(xg, 128)
        c2 = ops.farthest_point_sample(ops.index_points(xg, c1), 32)
        torch.manual_seed(31)
        ref_eval = model(xg)
    P = oracle.cast_params(state, torch.float64, requires_grad=False)
    with torch.no_grad():
        ref = oracle.vonmises_forward(xyz, P, [c1.cpu().long(), c2.cpu().long()], None, False, None)
    for g, r, e, n in zip(got, ref, ref_eval, ("mu", "kappa")):
        _gate_eval(g, r, f"fps {n}")
        print(f"  fps {n}: |predictor - model.eval()| = {float((g - e).abs().max()):.3e}")
    _features_case(oracle, model, state, xyz, [c1.cpu().long(), c2.cpu().long()], ((128, 32), (32, 32)), what="fps centres")


def test_ball_grouper_with_padded_neighbourhoods(oracle):
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    B, N, r = 4, 1024, 0.12
    model, state = _model(PointNetPPVonMises, grouper=("ball", r))
    xyz, _, _, _ = oracle.synthetic_clouds(B, N, seed=22)
    torch.manual_seed(8)
    c1, c2 = oracle.replay_centres(B)
    x1 = oracle.index_points(xyz, c1)
    n1 = oracle.ball_query(r, 32, xyz, x1)
    n2 = oracle.ball_query(r, 32, x1, oracle.index_points(x1, c2))
    padded = sum(int((n[..., 1:] == n[..., :1]).any(-1).sum()) for n in (n1, n2))
    print(f"  ball query r={r}: {padded} neighbourhoods padded with repeats of their first member")
    assert padded > 0
    routing = [{"neighbours": n1, "argmax": None}, {"neighbours": n2, "argmax": None}, {"neighbours": None, "argmax": None}]
    _features_case(oracle, model, state, xyz, [c1, c2], ((128, 32), (32, 32)), routing=routing, what="ball grouper")


def test_unsupported_k_takes_the_eval_path_bit_equal(oracle):
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    B, N = 4, 1024
    model, _ = _model(PointNetPPVonMises)
    model.sa1.nsample = 24
    p = Predictor(model)
    assert p.plan["sa1"] == "eval-path" and p.plan["sa2"] == "fused" and p.plan["sa3"] == "fused"
    xyz, _, _, _ = oracle.synthetic_clouds(B, N, seed=23)
    torch.manual_seed(9)
    centres = [c.cuda() for c in oracle.replay_centres(B)]
    with torch.no_grad():
        l1_f = p._level(0, xyz.cuda(), None, centres[0])
        l1_e = model.sa1(xyz.cuda(), None, centres[0])
        assert torch.equal(l1_f[0], l1_e[0]) and torch.equal(l1_f[1], l1_e[1])
        got, ref = p(xyz.cuda(), centres=centres), model(xyz.cuda(), centres=centres)
    for g, r in zip(got, ref):
        assert g.shape == r.shape and float((g - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max()))


def _whole_model(oracle, cls, fwd64, prep=None, B=32, N=1024, **fkw):
    from pnpp_hip.inference import Predictor
    torch.manual_seed(3)
    m = cls()
    if prep is not None:
        prep(m)
    _randomise(m, 103)
    state = _state(m)
    m = m.cuda().eval()
    p = Predictor(m)
    xyz, _, _, _ = oracle.synthetic_clouds(B, N, seed=1234)
    torch.manual_seed(7)
    centres = oracle.replay_centres(B)
    cg = [c.cuda() for c in centres]
    with torch.no_grad():
        got = p(xyz.cuda(), centres=cg)
        ev = m(xyz.cuda(), centres=cg)
        ref = fwd64(xyz, oracle.cast_params(state, torch.float64, requires_grad=False), centres, training=False, **fkw)
    torch.cuda.synchronize()
    return m, p, xyz, cg, got, ev, ref


def _as_tuple(t):
    return t if isinstance(t, (tuple, list)) else (t,)


def _compare(cls, got, ev, ref, angular=()):
    got, ev, ref = _as_tuple(got), _as_tuple(ev), _as_tuple(ref)
    assert type(got) is type(ev) and len(got) == len(ev) == len(ref)
    for i, (g, e, r) in enumerate(zip(got, ev, ref)):
        assert g.shape == e.shape and g.dtype == e.dtype and g.device == e.device and not g.requires_grad
        g64, r64 = g.detach().cpu().double(), r.detach().double().reshape(g.shape)
        if i in angular:   # angles: compare on the circle
            g64 = r64 + torch.remainder(g64 - r64 + math.pi, 2 * math.pi) - math.pi
        _gate_eval(g64, r64, f"{cls.__name__} output {i}")
        print(f"  {cls.__name__} output {i}: |predictor - model.eval()| = {float((g - e).abs().max()):.3e}")


def test_whole_model_vonmises(oracle):
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    _, _, _, _, got, ev, ref = _whole_model(oracle, PointNetPPVonMises, oracle.vonmises_forward)
    _compare(PointNetPPVonMises, got, ev, ref)   # mu = tanh(.) * pi: -pi and +pi are different outputs, compared directly


def test_whole_model_8dir(oracle):
    from models.pointnet_pp_8dir import PointNetPP8Dir
    _, _, _, _, got, ev, ref = _whole_model(oracle, PointNetPP8Dir, oracle.dir8_forward)
    _compare(PointNetPP8Dir, got, ev, ref)


def test_whole_model_fwd(oracle):
    from models.pointnet_pp_Fwd import PointNetPPFwd
    _, _, _, _, got, ev, ref = _whole_model(oracle, PointNetPPFwd, oracle.fwd_forward)
    _compare(PointNetPPFwd, got, ev, ref)


def test_whole_model_mvm_both_layouts(oracle):
    from models.pointnet_pp_mvM import PointNetPPMvM

    def prep(m):   # the zero-initialised pi / mu heads make every angle the degenerate fallback: move off it
        with torch.no_grad():
            torch.manual_seed(7)
            m.head_pi.weight.normal_(0, 0.05)
            m.head_mu.weight.normal_(0, 0.05)
            m.head_mu.bias.normal_(0, 0.05)

    m, p, xyz, cg, got, ev, ref = _whole_model(oracle, PointNetPPMvM, oracle.mvm_forward, prep=prep)
    assert p.plan["fc1"] == "eval-path" and p.plan["fc2"] == "eval-path" and p.plan["sa3"] == "fused"
    _compare(PointNetPPMvM, got, ev, ref, angular=(0,))
    with torch.no_grad():
        got_t = p(xyz.cuda().transpose(1, 2).contiguous(), centres=cg)
    for a, b in zip(got, got_t):
        assert torch.equal(a, b)


def test_forward_only_and_side_effect_free(oracle):
    from pnpp_hip import _lib, ops
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    B, N = 32, 1024
    model, _ = _model(PointNetPPVonMises)
    model.train()    # a Predictor evaluates in eval mode whatever mode the model is left in, and must not touch its statistics
    before = {k: v.clone() for k, v in model.state_dict().items()}
    p = Predictor(model)
    xyz = oracle.synthetic_clouds(B, N, seed=1234)[0].cuda()
    torch.manual_seed(7)
    cg = [c.cuda() for c in oracle.replay_centres(B)]
    outs = []
    for _ in range(3):
        outs.append([t.clone() for t in p(xyz, centres=cg)])
    torch.cuda.synchronize()
    mem = []
    for _ in range(2):   # the second and third call of this shape from here on: nothing accumulates
        p(xyz, centres=cg)
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
    after = model.state_dict()
    assert model.training
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b) and not a.requires_grad
    assert mem[0] == mem[1], mem
    # default sampler: the host generator advances by the model's own draws, in the same order
    model.eval()
    torch.manual_seed(123)
    with torch.no_grad():
        model(xyz)
    s_model = torch.get_rng_state()
    torch.manual_seed(123)
    p(xyz)
    assert torch.equal(torch.get_rng_state(), s_model)
    # no activation workspace: what the Predictor keeps is far below what the differentiable path keeps for backward
    lib = _lib.lib()
    saved = 0
    for sa, (n, s, k) in zip((model.sa1, model.sa2, model.sa3), ((N, 128, 32), (128, 32, 32), (32, 1, 32))):
        d = ops._sa_desc(B, n, s, k, sa.convs[0].weight.shape[1] - 3, [c.weight.shape[0] for c in sa.convs], sa.group_all, False, 1e-5, 0.1)
        saved += lib.pnpp_sa_saved_bytes(ctypes.byref(d))
    print(f"  persistent device memory {p.persistent_bytes()} bytes; saved workspaces of the three levels {saved} bytes")
    assert p.persistent_bytes() < saved


def test_refresh_after_a_training_step(oracle):
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    B, N = 32, 1024
    model, _ = _model(PointNetPPVonMises)
    p = Predictor(model)
    xyz, mu_gt, kappa_gt, _ = oracle.synthetic_clouds(B, N, seed=1234)
    torch.manual_seed(7)
    centres = oracle.replay_centres(B)
    cg = [c.cuda() for c in centres]
    first = [t.clone() for t in p(xyz.cuda(), centres=cg)]
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    mu, kappa = model(xyz.cuda(), centres=cg)
    ops.kl_von_mises_single(mu, kappa, mu_gt.cuda(), kappa_gt.cuda()).mean().backward()
    opt.step()
    model.eval()
    torch.cuda.synchronize()
    stale = p(xyz.cuda(), centres=cg)
    assert all(torch.equal(a, b) for a, b in zip(first, stale)), "a Predictor is a snapshot"
    with torch.no_grad():
        now = model(xyz.cuda(), centres=cg)
    assert any(float((a - b).abs().max()) > 1e-6 for a, b in zip(stale, now)), "the training step did not move the model"
    p.refresh()
    fresh = p(xyz.cuda(), centres=cg)
    P = oracle.cast_params(_state(model), torch.float64, requires_grad=False)
    with torch.no_grad():
        ref = oracle.vonmises_forward(xyz, P, centres, None, False, None)
    _compare(PointNetPPVonMises, fresh, now, ref)


def test_refused_at_call_time_runs_the_snapshot_and_says_so(oracle):
    """sa2.npoint changed after construction hands sa3 31 rows per cloud: `plan` (construction) says fused, the call runs sa3 on the
    eval path, `last_plan` says so, and the parameters are still the snapshot's, not the live model's."""
    from pnpp_hip.inference import Predictor
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    B, N = 4, 1024
    model, _ = _model(PointNetPPVonMises)
    p = Predictor(model)
    model.sa2.npoint = 31
    xyz = oracle.synthetic_clouds(B, N, seed=31)[0].cuda()
    torch.manual_seed(4)
    cg = [c.cuda() for c in oracle.replay_centres(B, sizes=((N, 128), (128, 31)))]
    with torch.no_grad():
        first = [t.clone() for t in p(xyz, centres=cg)]
        ref = model(xyz, centres=cg)
    assert p.plan["sa3"] == "fused" and p.last_plan["sa3"] == "eval-path" and p.last_plan["sa1"] == "fused"
    for a, b in zip(first, ref):
        assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max()))
    with torch.no_grad():
        for prm in model.sa3.parameters():
            prm.mul_(1.5)
    again = p(xyz, centres=cg)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "the refused level read the live model"
