"""GPU parity and contract of the Predictor's split-product attention (pnpp_attention_infer, csrc/attention_infer_kernels.hip) and of the
`attention=` keyword of pnpp_hip.transformer_inference.

The gate is this model's own (tests/test_gpu_pt.py, tests/test_gpu_pt_inference.py): |got - float64| <= 2e-5 * max(1, max|ref|).  For the
kernel alone the reference is float64 softmax attention on the kernel's own float32 input cast to float64; for the whole model it is
oracle.point_transformer_forward.  _stages() restates the few lines of tests/test_gpu_pt_inference.py that expose a layer's qkv.
Every case prints the float32 kernel's error on the same input next to the split kernel's.
"""
import ctypes
import math

import pytest
import torch

import dispatch

pytestmark = pytest.mark.gpu

GATE = 2e-5
H, DH, E = 4, 16, 64


def _pt_model(depth=6):
    """the model of tests/test_gpu_pt_inference.py::_pt_model (LayerNorm weights and biases moved off 1 / 0)"""
    from models.point_transformer import PointTransformer
    torch.manual_seed(42)
    m = PointTransformer(depth=depth)
    torch.manual_seed(5)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
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


def _qkv0(oracle, xyz, P, depth):
    """float64 qkv of layer 0, as _stages() of tests/test_gpu_pt_inference.py forms it; the oracle call checks the parameters' layout"""
    oracle.point_transformer_forward(xyz.double(), P, num_heads=H, depth=depth)
    x = xyz.double() @ P["input_proj.weight"].t() + P["input_proj.bias"]
    pre = "transformer.layers.0."
    return x @ P[pre + "self_attn.in_proj_weight"].t() + P[pre + "self_attn.in_proj_bias"]


def _attention64(qkv):
    """float64 softmax(q k^T / sqrt(d)) v per head on qkv (B, n, 3E) -> (B, n, E); also the scaled scores (B, H, n, n)"""
    qkv = qkv.double()
    B, n, _ = qkv.shape
    q, k, v = (t.reshape(B, n, H, DH).transpose(1, 2) for t in qkv.split(E, dim=-1))
    s = (q * (1.0 / math.sqrt(DH))) @ k.transpose(-1, -2)
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, n, E), s


def _err(got, ref):
    ref = ref.detach().cpu().double()
    return float((got.detach().cpu().double().reshape(ref.shape) - ref).abs().max()), GATE * max(1.0, float(ref.abs().max()))


def _check(what, got, ref, other=None):
    e, bound = _err(got, ref)
    tail = "" if other is None else f"; float32 kernel {_err(other, ref)[0]:.2e}"
    print(f"  {what}: |got - float64| = {e:.2e} (gate {bound:.2e}){tail}")
    assert e <= bound, (what, e, bound)


@pytest.fixture(scope="module")
def small():
    """the depth-2 model on the GPU, its float64 parameters and one Predictor per attention form"""
    from pnpp_hip import Predictor
    m = _pt_model(depth=2).cuda().eval()
    return m, _params64(m), Predictor(m, attention="split"), Predictor(m, attention="float32")


def _both(small, q32):
    """attend() of both forms on one float32 input; copies, the Predictors reuse their buffers"""
    _, _, ps, pf = small
    got = ps.attend(q32.cuda()).clone()
    assert ps.attention == "split" and ps.last_attention == "split"
    old = pf.attend(q32.cuda()).clone()
    assert pf.attention == "float32" and pf.last_attention == "float32"
    return got, old


@pytest.mark.parametrize("B, n_pts", [(1, 1), (2, 31), (2, 32), (2, 33), (1, 128), (2, 129), (3, 200), (2, 1000)])
def test_kernel_alone(small, oracle, B, n_pts):
    """one key and 127 padded queries (1); the -inf masking inside a key block and a block boundary (31, 32, 33); no padding (128); a
    query tile with one real row and a key block with one real key (129); 200; many key blocks and the online rescale (1000)"""
    _, P, _, _ = small
    q32 = _qkv0(oracle, _cloud(B, n_pts, seed=200 + n_pts), P, 2).float()
    ref, _ = _attention64(q32)
    got, old = _both(small, q32)
    N = (n_pts + 127) // 128 * 128
    assert got.shape == (B, N, E) and got.dtype == torch.float32
    print()
    _check(f"attend {B} x {n_pts}", got[:, :n_pts], ref, old[:, :n_pts])
    assert bool(torch.isfinite(got).all()), "padded query rows must be finite"


def _stress_qkv(first_block_holds_the_maximum):
    """B = 1, n = 160 (five key blocks of 32), synthetic: dim 0 of every head carries the score, q_0 in [2, 2.5] and k_0 stepping up by
    6 from block to block with a spread of 2 inside a block, the other dims are small noise; v is N(0, 1)"""
    n, g = 160, torch.Generator().manual_seed(77)
    q = 0.1 * torch.randn(1, n, H, DH, generator=g)
    k = 0.1 * torch.randn(1, n, H, DH, generator=g)
    v = torch.randn(1, n, H, DH, generator=g)
    q[..., 0] = 2.0 + 0.5 * torch.rand(1, n, H, generator=g)
    block = torch.arange(n) // 32
    if first_block_holds_the_maximum:
        block = 4 - block
    k[..., 0] = (-14.0 + 6.0 * block.double()).float()[None, :, None] + 2.0 * torch.rand(1, n, H, generator=g)
    return torch.cat([q.reshape(1, n, E), k.reshape(1, n, E), v.reshape(1, n, E)], dim=-1)


@pytest.mark.parametrize("first", [False, True], ids=["rising-maximum", "maximum-in-first-block"])
def test_rescale_stress(small, first):
    """the running maximum of every query rises in each of the five key blocks (alpha < 1 four times), or sits in the first block
    (alpha = 1 thereafter: the wave-uniform branch that skips the rescale).  Scaled scores within +-10: their float32 rounding is about
    1e-6, a twentieth of the gate."""
    q32 = _stress_qkv(first)
    ref, s = _attention64(q32)
    assert float(s.abs().max()) <= 10.0, float(s.abs().max())
    bm = s.reshape(1, H, 160, 5, 32).max(dim=-1).values   # per query, the maximum of each key block
    if first:
        assert bool((bm[..., 0:1] > bm[..., 1:]).all())
    else:
        assert bool((bm[..., 1:] > bm[..., :-1]).all())
    got, old = _both(small, q32)
    print()
    _check("rescale stress, " + ("maximum in the first block" if first else "maximum rising in every block"), got[:, :160], ref, old[:, :160])
    assert bool(torch.isfinite(got).all())


def test_deterministic_and_independent_of_the_padding(small):
    from pnpp_hip import _lib as L, ops
    _, _, ps, _ = small
    g = torch.Generator().manual_seed(5)
    B, N, n_valid = 2, 256, 161
    q32 = torch.randn(B, n_valid, 3 * E, generator=g).cuda()
    a = ps.attend(q32).clone()
    b = ps.attend(q32).clone()
    assert torch.equal(a, b)
    # the entry point itself at a fixed n_valid: rows at or beyond it hold zeros, then large finite values
    qkv = torch.zeros(B, N, 3 * E, device="cuda")
    qkv[:, :n_valid] = q32
    out0, out1 = torch.empty(B, N, E, device="cuda"), torch.empty(B, N, E, device="cuda")
    L.check(L.lib().pnpp_attention_infer(qkv.data_ptr(), B, N, n_valid, H, DH, out0.data_ptr(), ops._stream()))
    qkv[:, n_valid:] = 1e4
    L.check(L.lib().pnpp_attention_infer(qkv.data_ptr(), B, N, n_valid, H, DH, out1.data_ptr(), ops._stream()))
    torch.cuda.synchronize()
    assert torch.equal(out0[:, :n_valid], a[:, :n_valid])
    assert torch.equal(out1[:, :n_valid], out0[:, :n_valid])
    assert bool(torch.isfinite(out1).all())


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


@pytest.fixture(scope="module")
def deep():
    from pnpp_hip import Predictor
    m = _pt_model(depth=6).cuda().eval()
    return m, _params64(m), {form: Predictor(m, attention=form) for form in ("split", "float32")}


@pytest.mark.parametrize("B, n_pts", [(2, 1024), (3, 200)])
def test_whole_model_vs_oracle(deep, oracle, B, n_pts):
    _, P, preds = deep
    xyz = _cloud(B, n_pts, seed=3)
    ref = oracle.point_transformer_forward(xyz.double(), P)
    print()
    for form, p in preds.items():
        out = p(xyz.cuda())
        assert out.shape == (B, 3) and p.last_attention == form and set(p.last_plan.values()) == {"fused"}
        _check(f"predictor, attention={form!r}", out, ref)


def test_dispatch_and_launch_count(deep):
    _, _, preds = deep
    depth = 6
    xyz = _cloud(2, 300, seed=4).cuda()
    for form, p in preds.items():
        p(xyz)
        tags = dispatch.record(lambda: p(xyz))
        mine = _counts(lambda: p(xyz))
        new = sum(n for t, n in mine.items() if t.startswith("attention_fwd_kernel<split>"))
        old = sum(n for t, n in mine.items() if t.startswith("attention_fwd_kernel "))
        print(f"\n  attention={form!r}: {sum(mine.values())} launches, attention tags {dispatch.find(tags, 'attention_fwd_kernel')}")
        assert sum(mine.values()) == 2 + 2 * depth, mine
        assert (new, old) == ((depth, 0) if form == "split" else (0, depth)), mine
        dispatch.expect(tags, present=["attention_fwd_kernel", "pt_tail_infer_kernel M=768 E=64 F=2048"], absent=["add_layernorm_kernel", "gemm_"])
        assert bool(dispatch.find(tags, "attention_fwd_kernel<split> B=2 N=384 H=4")) == (form == "split")


def test_fallback_runs_the_float32_kernel_and_says_so(small, oracle):
    """Every call the fused path takes (pnpp_pt_infer_supported: H = 4, head dimension 16, N a multiple of 128, 1 <= n_valid <= N) is one
    pnpp_attention_infer takes as well, which the first half asserts over the sizes; so the fall-back has no natural trigger, and the
    second half makes the Predictor's query answer no for one call."""
    from pnpp_hip import _lib as L
    model, P, ps, _ = small
    for B in (1, 7, 64):
        for n_pts in (1, 128, 129, 5000):
            N = (n_pts + 127) // 128 * 128
            d = ps._desc(B, N, n_pts)
            assert L.lib().pnpp_pt_infer_supported(ctypes.byref(d)) == 1
            assert ps._split_supported(d), L.last_error()
    xyz = _cloud(2, 200, seed=8)
    ref = oracle.point_transformer_forward(xyz.double(), P, depth=2)
    split = ps(xyz.cuda())
    assert ps.last_attention == "split"
    ps._split_supported = lambda d: False
    try:
        tags = dispatch.record(lambda: ps(xyz.cuda()))
        out = ps(xyz.cuda())
        assert ps.attention == "split" and ps.last_attention == "float32"
        assert not dispatch.find(tags, "attention_fwd_kernel<split>") and dispatch.find(tags, "attention_fwd_kernel B=2 N=256 H=4")
    finally:
        del ps._split_supported
    print()
    _check("fall-back call", out, ref)
    _check("split call", split, ref)
    assert torch.equal(ps(xyz.cuda()), split) and ps.last_attention == "split"
