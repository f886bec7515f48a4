"""GPU parity and contract of the forward-only path of the point transformer (pnpp_hip.transformer_inference, csrc/transformer_infer_kernels.hip).

The gate is the one this model's kernels carry in tests/test_gpu_pt.py: |got - float64| <= 2e-5 * max(1, max|ref|), the float64 reference
oracle.point_transformer_forward(..., return_layers=True).  _stages() below restates that function layer by layer only to expose the
tensors it does not return (a layer's qkv and attention output): every layer's input and output there are the oracle's own.
"""
import ctypes
import math

import pytest
import torch

import dispatch

pytestmark = pytest.mark.gpu

GATE = 2e-5


def _pt_model(depth=6, shift_norms=True, **kw):
    """randomised as tests/test_gpu_pt.py::_pt_model; the LayerNorm weights and biases moved off 1 / 0"""
    from models.point_transformer import PointTransformer
    torch.manual_seed(42)
    m = PointTransformer(depth=depth, **kw)
    torch.manual_seed(5)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
        if shift_norms:
            g = torch.Generator().manual_seed(11)
            for mod in m.modules():
                if isinstance(mod, torch.nn.LayerNorm):
                    mod.weight.add_(0.3 * torch.randn(mod.weight.shape, generator=g))
                    mod.bias.add_(0.3 * torch.randn(mod.bias.shape, generator=g))
    return m


def _cloud(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, n, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 0.6, 0.3])


def _params64(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


def _stages(oracle, xyz, P, depth, H=4):
    """float64: per layer the input x, qkv, the attention output o (in front of out_proj) and the output; checked against the oracle"""
    out, layers = oracle.point_transformer_forward(xyz.double(), P, num_heads=H, depth=depth, return_layers=True)
    x = xyz.double() @ P["input_proj.weight"].t() + P["input_proj.bias"]
    B, N, E = x.shape
    dh = E // H
    st = []
    for l in range(depth):
        pre = f"transformer.layers.{l}."
        qkv = x @ P[pre + "self_attn.in_proj_weight"].t() + P[pre + "self_attn.in_proj_bias"]
        q, k, v = (t.reshape(B, N, H, dh).transpose(1, 2) for t in qkv.split(E, dim=-1))
        att = torch.softmax((q * (1.0 / math.sqrt(dh))) @ k.transpose(-1, -2), dim=-1)
        o = (att @ v).transpose(1, 2).reshape(B, N, E)
        st.append({"x": x, "qkv": qkv, "o": o, "y": layers[l]})
        x = layers[l]
    return out, st


def _err(got, ref):
    """(max abs difference, the gate's bound)"""
    ref = ref.detach().cpu().double()
    return float((got.detach().cpu().double().reshape(ref.shape) - ref).abs().max()), GATE * max(1.0, float(ref.abs().max()))


def _check(what, got, ref):
    e, bound = _err(got, ref)
    print(f"  {what}: |got - float64| = {e:.2e} (gate {bound:.2e})")
    assert e <= bound, (what, e, bound)


@pytest.fixture(scope="module")
def small():
    """the depth-2 model of most cases, on the GPU, with its float64 parameters"""
    m = _pt_model(depth=2).cuda().eval()
    return m, _params64(m)


def test_fold_is_exact(small):
    from pnpp_hip import Predictor
    model, _ = small
    p = Predictor(model)
    assert p.plan == {"head": "fused", "layers.0": "fused", "layers.1": "fused", "pool": "fused"}
    for l, layer in enumerate(model.transformer.layers):
        att = layer.self_attn
        for name, w, b in (("in_proj", att.in_proj_weight, att.in_proj_bias), ("out_proj", att.out_proj.weight, att.out_proj.bias),
                           ("linear1", layer.linear1.weight, layer.linear1.bias), ("linear2", layer.linear2.weight, layer.linear2.bias),
                           ("norm1", layer.norm1.weight, layer.norm1.bias), ("norm2", layer.norm2.weight, layer.norm2.bias)):
            fw, fb = p.folded(l, name)
            assert torch.equal(fw, w.detach()) and torch.equal(fb, b.detach()), (l, name)   # the three-way split loses nothing
    fw, fb = p.folded(0, "input_proj")
    assert fw.shape == (64, 8) and torch.equal(fw[:, :3], model.input_proj.weight.detach()) and torch.equal(fb, model.input_proj.bias.detach())
    assert float(fw[:, 3:].abs().max()) == 0.0   # the padding columns


@pytest.mark.parametrize("B, n_pts", [(1, 128), (2, 200), (3, 1000), (1, 1), (2, 129)])
def test_tail_kernel_alone(small, oracle, B, n_pts):
    """a layer's tail on float64's own x and attention output: a fully padded tile (1 point, 129 points), a tile straddling n_valid
    (200, 1000), a cloud of one point"""
    from pnpp_hip import Predictor, ops, transformer as T
    model, P = small
    p = Predictor(model)
    xyz = _cloud(B, n_pts, seed=100 + n_pts)
    out64, st = _stages(oracle, xyz, P, 2)
    print()
    for l in (0, 1):
        x32, o32 = st[l]["x"].float().cuda(), st[l]["o"].float().cuda()
        x_next, second = p.tail(l, x32, o32)
        _check(f"layer {l} x_next", x_next[:, :n_pts], st[l]["y"])
        if l == 0:
            _check("layer 0 qkv_next", second[:, :n_pts], st[1]["qkv"])
        else:
            _check("layer 1 pooled mean", second, st[1]["y"].mean(dim=1))
        # the existing eval-path operators on the same inputs (printed, not gated here)
        layer = model.transformer.layers[l]
        with torch.no_grad():
            a = ops.fc_block(o32.view(B * n_pts, 64), layer.self_attn.out_proj, training=False)
            u = T.add_layernorm(x32.view(B * n_pts, 64), a, layer.norm1)
            f = ops.fc_block(ops.fc_block(u, layer.linear1, relu=True, training=False), layer.linear2, training=False)
            y = T.add_layernorm(u, f, layer.norm2)
        print(f"  layer {l} eval-path operators: |y - float64| = {_err(y.view(B, n_pts, 64), st[l]['y'])[0]:.2e}")


@pytest.mark.parametrize("B, n_pts", [(2, 200), (1, 1)])
def test_head_kernel(small, oracle, B, n_pts):
    from pnpp_hip import Predictor
    model, P = small
    p = Predictor(model)
    xyz = _cloud(B, n_pts, seed=7)
    _, st = _stages(oracle, xyz, P, 2)
    x0, qkv0 = p.head(xyz.cuda())
    print()
    _check("x0", x0[:, :n_pts], st[0]["x"])
    _check("qkv_0", qkv0[:, :n_pts], st[0]["qkv"])
    N = x0.shape[1]
    assert N % 128 == 0 and N >= n_pts
    # padding rows are what a zero point gives
    zero = torch.zeros(1, 1, 3)
    _, z = _stages(oracle, zero, P, 2)
    _check("x0 padding rows", x0[:, n_pts:], z[0]["x"].expand(B, N - n_pts, 64))
    _check("qkv_0 padding rows", qkv0[:, n_pts:], z[0]["qkv"].expand(B, N - n_pts, 192))
    assert torch.equal(x0[:, n_pts:], x0[:1, n_pts:n_pts + 1].expand(B, N - n_pts, 64))


def test_whole_model_matches_reference_capture(golden):
    from pnpp_hip import Predictor
    g = golden("pt.npz")
    model = _pt_model(shift_norms=False).cuda().eval()   # the model the fixture was captured from
    xyz = torch.from_numpy(g["xyz"]).cuda()
    p = Predictor(model)
    out = p(xyz)
    assert p.last_plan == p.plan and set(p.plan.values()) == {"fused"}
    with torch.no_grad():
        ev = model(xyz)
    print(f"\n  |predictor - model.eval()| = {float((out - ev).abs().max()):.2e}")
    _check("predictor vs the reference's float64 capture", out, torch.from_numpy(g["pt_f64.eval_out"]))


@pytest.mark.parametrize("B, n_pts", [(2, 1024), (3, 200)])
def test_whole_model_vs_oracle(oracle, B, n_pts):
    from pnpp_hip import Predictor
    model = _pt_model().cuda().eval()
    xyz = _cloud(B, n_pts, seed=3)
    ref = oracle.point_transformer_forward(xyz.double(), _params64(model))
    p = Predictor(model)
    out = p(xyz.cuda())
    assert out.shape == (B, 3) and out.dtype == torch.float32 and out.is_cuda and not out.requires_grad
    with torch.no_grad():
        ev = model(xyz.cuda())
    print(f"\n  |predictor - model.eval()| = {float((out - ev).abs().max()):.2e}; |model.eval() - float64| = {_err(ev, ref)[0]:.2e}")
    _check("predictor", out, ref)


def _counts(fn):
    """{tag: launches} of one call, through pnpp_profile_report"""
    from pnpp_hip import _lib
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.pnpp_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 18)
        assert lib.pnpp_profile_report(buf, len(buf)) >= 0
    finally:
        lib.pnpp_profile_enable(0)
    return {ln.split("\t")[0]: int(ln.split("\t")[1]) for ln in buf.value.decode().splitlines()}


def test_dispatch():
    from pnpp_hip import Predictor
    depth = 6
    model = _pt_model().cuda().eval()
    xyz = _cloud(2, 300, seed=4).cuda()
    p = Predictor(model)
    p(xyz)

    def run_eval():
        with torch.no_grad():
            model(xyz)
    run_eval()
    tags = dispatch.record(lambda: p(xyz))
    wide = [t for t in tags if "N=2048" in t.split() or "K=2048" in t.split()]
    assert not wide, wide
    dispatch.expect(tags, present=["pt_head_infer_kernel M=768 E=64 F=2048", "pt_pool_infer_kernel M=768 E=64 F=2048",
                                   "pt_tail_infer_kernel M=768 E=64 F=2048", "attention_fwd_kernel"],
                    absent=["add_layernorm_kernel", "mean_points_kernel", "linear_smallk_kernel", "gemm_"])
    assert len(dispatch.find(tags, "pt_head_infer_kernel")) == 1 and len(dispatch.find(tags, "pt_pool_infer_kernel")) == 1
    ev_tags = dispatch.record(run_eval)
    dispatch.expect(ev_tags, present=["add_layernorm_kernel", "mean_points_kernel", "linear_smallk_kernel", "attention_fwd_kernel"],
                    absent=["pt_head_infer_kernel", "pt_tail_infer_kernel", "pt_pool_infer_kernel"])
    assert [t for t in ev_tags if "N=2048" in t.split() or "K=2048" in t.split()], ev_tags
    mine, theirs = _counts(lambda: p(xyz)), _counts(run_eval)
    print(f"\n  launches per forward: predictor {sum(mine.values())}, model.eval() {sum(theirs.values())}")
    assert sum(mine.values()) == 2 + 2 * depth, mine
    assert sum(n for t, n in mine.items() if t.startswith("pt_tail_infer_kernel")) == depth
    assert sum(n for t, n in mine.items() if t.startswith("attention_fwd_kernel")) == depth
    assert sum(mine.values()) < sum(theirs.values())


def test_largest_allocation_of_a_call():
    """bytes (the torch.empty spy of tests/test_gpu_pointnet_inference.py): nothing the Predictor allocates is larger than the qkv buffer,
    and a call's allocations together stay far below one B*N x F float32 tensor"""
    from pnpp_hip import Predictor
    B, N, E, F = 4, 1024, 64, 2048
    model = _pt_model(depth=2).cuda().eval()
    x = _cloud(B, N, seed=6).cuda()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    sizes = []
    empty = torch.empty

    def spy(*shape, **kw):
        t = empty(*shape, **kw)
        if t.is_cuda:
            sizes.append(t.numel() * t.element_size())
        return t

    torch.empty = spy
    try:
        p = Predictor(model)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        p(x)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    finally:
        torch.empty = empty
    print(f"\n  largest torch.empty of construction + one call: {max(sizes)} bytes; peak above the baseline {peak} bytes")
    assert max(sizes) <= B * N * 3 * E * 4
    assert peak < B * N * F * 4
    assert all(t.shape[-1] < F for t in p._bufs.values() if t.dtype == torch.float32)


def test_contract(oracle):
    from pnpp_hip import Predictor, ops
    B, n_pts = 2, 300
    model = _pt_model(depth=2).cuda().train()   # left in train mode: the dropouts are live for model(xyz)
    xyz = _cloud(B, n_pts, seed=9)
    xg = xyz.cuda().requires_grad_(True)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    p = Predictor(model)
    a = p(xg)
    b = p(xg)
    assert torch.equal(a, b)
    del b
    torch.cuda.synchronize()
    m2 = torch.cuda.memory_allocated()
    c = p(xg)
    assert torch.equal(a, c)
    del c
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m2   # buffers are reused: the third call allocates nothing that stays
    assert not a.requires_grad and a.grad_fn is None
    assert model.training and all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    print()
    _check("train-mode model, eval-mode value", a, oracle.point_transformer_forward(xyz.double(), _params64(model), depth=2))
    assert p.persistent_bytes() == sum(t.numel() * t.element_size() for t in p.held_tensors()) > 0
    # a snapshot: stale after an optimiser step, right again after refresh()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    model.set_dropout(0.0)
    ops.mse_loss(model(xyz.cuda()), torch.zeros(B, 3, device="cuda")).backward()
    opt.step()
    assert torch.equal(p(xg), a)
    new64 = oracle.point_transformer_forward(xyz.double(), _params64(model), depth=2)
    assert _err(a, new64)[0] > 10 * _err(a, new64)[1], "the step did not move the output: the staleness check shows nothing"
    p.refresh()
    _check("after refresh()", p(xg), new64)


def _refused_models():
    from models.point_transformer import PointTransformer
    torch.manual_seed(1)
    wide = PointTransformer(embed_dim=128, num_heads=8, depth=2)
    torch.manual_seed(2)
    narrow = PointTransformer(depth=2)
    for layer in narrow.transformer.layers:
        layer.linear1, layer.linear2 = torch.nn.Linear(64, 96), torch.nn.Linear(96, 64)
    return {"E=128": wide, "F=96": narrow}


@pytest.mark.parametrize("which", ["E=128", "F=96"])
def test_refused_models_run_the_eval_path_on_the_snapshot(which):
    from pnpp_hip import Predictor
    model = _refused_models()[which].cuda().eval()
    xyz = _cloud(2, 200, seed=12).cuda()
    p = Predictor(model)
    assert set(p.plan) == {"head", "layers.0", "layers.1", "pool"} and set(p.plan.values()) == {"eval-path"}
    assert which in p.refused
    with torch.no_grad():
        ref = model(xyz)
    out = p(xyz)
    assert set(p.last_plan.values()) == {"eval-path"}
    assert torch.equal(out, ref) and not out.requires_grad
    tags = dispatch.record(lambda: p(xyz))
    dispatch.expect(tags, present=["add_layernorm_kernel", "attention_fwd_kernel"], absent=["pt_tail_infer_kernel", "pt_head_infer_kernel"])
    with torch.no_grad():
        for q in model.parameters():
            q.mul_(1.5)
        moved = model(xyz)
    assert not torch.equal(moved, ref)
    assert torch.equal(p(xyz), ref)      # the snapshot, not the live model
    p.refresh()
    assert torch.equal(p(xyz), moved)
