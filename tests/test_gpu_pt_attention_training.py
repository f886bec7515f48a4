"""GPU parity and contract of the point transformer's TRAINING attention on the bf16 matrix pipe (pnpp_attention_split_fwd / _split_bwd,
csrc/attention_train_kernels.hip), reached through pnpp_hip.transformer.attention(form="split") and PointTransformer.set_attention.

The yardstick is tests/test_gpu_pt_bands.py's: float64 softmax attention on the kernel's own float32 inputs with the same keep bits, out
and dqkv within ATT_GATE * max(1, max|ref|), lse within ATT_GATE absolute, padding rows of dqkv exactly zero.  Every band case runs in
both forms and prints the two errors side by side (printed, not gated: the gate is the project's existing one).
"""
import ctypes

import pytest
import torch

import dispatch
from test_gpu_pt import _pt_model, _unpack
from test_gpu_pt_attention_inference import _stress_qkv
from test_gpu_pt_bands import ATT_CASES, ATT_GATE, _att_inputs, _attention64, _check_attention, _masks, _maxerr, _padded

pytestmark = pytest.mark.gpu

# the boundaries of the split kernels' 64-wide stages: one key short of a stage, a full stage, one key into the second tile's stage; a
# stage whose second 32-key tile holds no point (160 = 2 * 64 + 32); one key into a fourth stage
STAGE_CASES = [(1, 128, 2, 63, 0.25), (1, 128, 2, 64, 0.0), (2, 128, 2, 65, 0.25), (1, 256, 4, 160, 0.0), (1, 256, 4, 193, 0.25)]


def _run(qkv, up, H, p, masks, nv, form):
    """forward and backward on the padded layout (B, N, 3E) -> out (B, N, E), lse (B, H, N), dqkv (B, N, 3E), on the CPU"""
    from pnpp_hip import transformer as T
    qg = qkv.clone().cuda().requires_grad_(True)
    out, lse = T.attention(qg, H, want_lse=True, p=p, masks=masks, n_valid=nv, form=form)
    (out * up.cuda()).sum().backward()
    return out.detach().cpu(), lse.cpu(), qg.grad.cpu()


def _errors(got, ref, nv):
    return _maxerr(got[0][:, :nv], ref[0]), _maxerr(got[1][..., :nv], ref[1]), _maxerr(got[2][:, :nv], ref[2])


@pytest.mark.parametrize("B,N,H,nv,p", ATT_CASES + STAGE_CASES)
def test_attention_bands_split(B, N, H, nv, p):
    qkv, up = _att_inputs(B, H, nv, 1000 * N + nv)
    masks = _masks(B, N, H, p)
    keep = _unpack(masks[0], N)[:, :, :nv, :nv] if masks is not None else None
    ref = _attention64(qkv, H, up, keep, p)
    got = _run(_padded(qkv, N), _padded(up, N), H, p, masks, nv, "split")
    old = _run(_padded(qkv, N), _padded(up, N), H, p, masks, nv, "float32")
    es, ef = _errors(got, ref, nv), _errors(old, ref, nv)
    print(f"\n[forms B{B} N{N} H{H} nv{nv} p{p}] |got - float64| out / lse / dqkv:  split {es[0]:.2e} {es[1]:.2e} {es[2]:.2e}   "
          f"float32 {ef[0]:.2e} {ef[1]:.2e} {ef[2]:.2e}")
    _check_attention(f"split B{B} N{N} H{H} nv{nv} p{p}", got, ref, nv)
    again = _run(_padded(qkv, N), _padded(up, N), H, p, masks, nv, "split")
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_split_attention_is_independent_of_the_padding(p):
    """tests/test_gpu_pt_bands.py::test_attention_is_independent_of_the_padding in the split form: padding rows of qkv at zero, then
    at 1e4; everything finite, what the valid rows receive bit-equal, the padded rows of dqkv zero."""
    B, N, H, nv = 2, 256, 4, 161
    qkv, up = _att_inputs(B, H, nv, 5)
    masks = _masks(B, N, H, p)
    zero = _run(_padded(qkv, N), _padded(up, N), H, p, masks, nv, "split")
    big = _padded(qkv, N)
    big[:, nv:] = 1e4
    large = _run(big, _padded(up, N), H, p, masks, nv, "split")
    nonfinite = [int((~torch.isfinite(t)).sum()) for t in large]
    print(f"\n[split attention, padding at 1e4, p {p}] non-finite elements of out / lse / dqkv: {nonfinite}")
    assert nonfinite == [0, 0, 0], nonfinite
    assert all(bool(torch.isfinite(t).all()) for t in zero)
    assert torch.equal(large[0][:, :nv], zero[0][:, :nv])
    assert torch.equal(large[1][..., :nv], zero[1][..., :nv])
    assert torch.equal(large[2][:, :nv], zero[2][:, :nv])
    assert bool((large[2][:, nv:] == 0).all()) and bool((zero[2][:, nv:] == 0).all())


@pytest.mark.parametrize("first", [False, True], ids=["rising-maximum", "maximum-in-first-block"])
def test_split_attention_rescale_stress(first):
    """n = 160 padded to 256: the running maximum of every query rises in each 32-key tile (the rescale branch taken in every tile of
    every stage) or sits in the first one (alpha = 1 thereafter).  Scaled scores within +-10: their float32 rounding is about 1e-6."""
    H, n, N = 4, 160, 256
    qkv = _stress_qkv(first)
    up = torch.randn(1, n, 16 * H, generator=torch.Generator().manual_seed(78))
    ref = _attention64(qkv, H, up)
    s = ref[3]
    assert float(s.abs().max()) <= 10.0, float(s.abs().max())
    bm = s.reshape(1, H, n, 5, 32).max(dim=-1).values
    assert bool((bm[..., 0:1] > bm[..., 1:]).all()) if first else bool((bm[..., 1:] > bm[..., :-1]).all())
    got = _run(_padded(qkv, N), _padded(up, N), H, 0.0, None, n, "split")
    _check_attention("split, rescale stress, " + ("maximum in the first block" if first else "maximum rising in every block"), got, ref, n)
    assert all(bool(torch.isfinite(t).all()) for t in got)


def test_split_lse_does_not_see_the_mask():
    """The softmax denominator is the sum of the UNDROPPED probabilities: lse of the masked call is bit-equal to lse of the unmasked call
    on the same qkv, while out differs."""
    from pnpp_hip import transformer as T
    B, N, H, nv, p = 2, 256, 4, 193, 0.25
    qkv, _ = _att_inputs(B, H, nv, 9)
    q = _padded(qkv, N).cuda()
    out0, lse0 = T.attention(q, H, want_lse=True, n_valid=nv, form="split")
    out1, lse1 = T.attention(q, H, want_lse=True, p=p, masks=_masks(B, N, H, p), n_valid=nv, form="split")
    assert torch.equal(lse0, lse1)
    assert not torch.equal(out0[:, :nv], out1[:, :nv])


def test_whole_model_split_vs_oracle(oracle):
    """tests/test_gpu_pt.py::test_point_transformer_any_cloud_size with set_attention("split"): three clouds of 200 points, depth 6, train
    mode with dropout 0 and an MSE loss against float64 autograd of the restatement, under that test's gates."""
    from pnpp_hip import ops
    import synthetic
    n = 200
    model = _pt_model()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    xyz, _, _, fwd = synthetic.rotated_clouds(3, n, seed=n)
    model = model.cuda().train().set_dropout(0.0).set_attention("split")
    out = model(xyz.cuda())
    loss = ops.mse_loss(out, fwd.cuda())
    loss.backward()
    P64 = oracle.cast_params(state, torch.float64)
    ref = oracle.point_transformer_forward(xyz.double(), P64)
    l64 = ((ref - fwd.double()) ** 2).mean()
    l64.backward()
    scale = max(1.0, float(ref.detach().abs().max()))
    e_out, e_loss = float((out.detach().cpu().double() - ref.detach()).abs().max()), abs(loss.item() - float(l64.detach()))
    worst = 0.0
    for name, p in model.named_parameters():
        r = P64[name].grad.reshape(p.shape)
        worst = max(worst, float((p.grad.detach().cpu().double() - r).norm() / r.norm().clamp_min(1e-30)))
    print(f"\n[PT split, 3 x {n}] out {e_out:.2e} (gate {2e-5 * scale:.2e})  loss {e_loss:.2e} (gate {1e-5 * max(1.0, float(l64.detach())):.2e})  "
          f"worst per-tensor gradient relL2 {worst:.2e} (gate 1e-03)")
    assert e_out <= 2e-5 * scale
    assert e_loss <= 1e-5 * max(1.0, float(l64.detach()))
    assert worst <= 1e-3, worst
    model.set_dropout(0.1)                                    # one step with the default dropout runs and is finite
    model.zero_grad()
    ops.mse_loss(model(xyz.cuda()), fwd.cuda()).backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def _counts(fn):
    """{tag: launches} of one call, through pnpp_profile_report (as tests/test_gpu_pt_attention_inference.py)"""
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


SPLIT_TAGS = ("attention_fwd_kernel<split,train>", "attention_bwd_dq_kernel<split>", "attention_bwd_dkv_kernel<split>")
FLOAT_TAGS = ("attention_fwd_kernel ", "attention_bwd_dq_kernel ", "attention_bwd_dkv_kernel ")


def test_dispatch_follows_the_form():
    from pnpp_hip import ops
    import synthetic
    depth = 6
    xyz, _, _, fwd = synthetic.rotated_clouds(2, 200, seed=3)
    xyz, fwd = xyz.cuda(), fwd.cuda()

    def step(model):
        model.zero_grad()
        ops.mse_loss(model(xyz), fwd).backward()

    def per_tag(mine, tags):
        return [sum(n for t, n in mine.items() if t.startswith(tag)) for tag in tags]

    plain = _pt_model().cuda().train().set_dropout(0.0)       # never calls set_attention
    step(plain)
    before = _counts(lambda: step(plain))
    assert per_tag(before, FLOAT_TAGS) == [depth] * 3 and per_tag(before, SPLIT_TAGS) == [0] * 3, before
    model = _pt_model().cuda().train().set_dropout(0.0).set_attention("split")
    step(model)
    mine = _counts(lambda: step(model))
    tags = dispatch.record(lambda: step(model))
    print(f"\n  set_attention('split'): {sum(mine.values())} launches, attention tags {dispatch.find(tags, 'attention_')}")
    assert per_tag(mine, SPLIT_TAGS) == [depth] * 3 and per_tag(mine, FLOAT_TAGS) == [0] * 3, mine
    assert dispatch.find(tags, "attention_fwd_kernel<split,train> B=2 N=256 H=4")
    # everything else is launched exactly as without set_attention
    rest = lambda c: {t: n for t, n in c.items() if not t.startswith("attention_")}
    assert rest(mine) == rest(before)
    back = _counts(lambda: step(model.set_attention("float32")))
    assert back == before


def test_split_form_refuses_what_the_library_refuses():
    from pnpp_hip import transformer as T
    qkv = torch.zeros(1, 128, 3 * 32, device="cuda")
    with pytest.raises(ValueError, match="head_dim=32"):
        T.attention(qkv, 1, form="split")
