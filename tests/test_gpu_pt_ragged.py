"""Ragged batches of the point transformer: a padded tensor plus a per-cloud lengths tensor, through the attention kernels (float32,
split, infer), mean_points, the model in eval and train mode, and the Predictor's fused kernels.

One shape family: H = 4, head dimension 16, E = 64, B = 12, N = 384.  The kernel-level lengths sit on both sides of every edge the
kernels have -- the 32-key block, the 64-row stage, the 128-query workgroup -- and include a full cloud, clouds with one and with two
wholly padded query workgroups, and a single point.  At model level n_pts = 300 (rows padded to 384), so the first length is 300.

Yardsticks: the existing uniform call on one cloud alone with n_valid = the cloud's length (bit equality: the same kernel, the same N,
the same Nv, the same block order, no atomics), tests/test_gpu_pt_bands.py's float64 attention under its ATT_GATE, and float64 stock
modules (the model's own containers, deep-copied to double on the CPU) on each cloud alone and unpadded, under the gates of
tests/test_gpu_pt_attention_training.py.
"""
import copy
import functools

import pytest
import torch

from test_gpu_pt import _pt_model, _unpack
from test_gpu_pt_bands import ATT_GATE, _attention64, _check_attention, _maxerr

pytestmark = pytest.mark.gpu

H, E, B, N = 4, 64, 12, 384
LENS = [384, 257, 256, 129, 128, 127, 65, 64, 33, 32, 31, 1]
N_PTS = 300
MODEL_LENS = [N_PTS] + LENS[1:]
FORMS = ("float32", "split")


# ------------------------------------------------------------------------------------------------ kernel level
@functools.lru_cache(maxsize=None)
def _inputs():
    """qkv (B, N, 3E) and an upstream gradient (B, N, E), random in EVERY row: the padding rows hold finite values that must not matter"""
    g = torch.Generator().manual_seed(384)
    qkv = torch.randn(B, N, 3 * E, generator=g) * 1.5
    qkv[0, :, :E] *= 3.0                                      # a cloud with peaked softmax rows
    return qkv, torch.randn(B, N, E, generator=g)


@functools.lru_cache(maxsize=None)
def _masks(p):
    from pnpp_hip import transformer as T
    return T.attention_dropout_mask(B, N, H, p, "cuda", seed=11, stream_id=3) if p > 0 else None


def _zero_padding(t, lens):
    t = t.clone()
    for b, n in enumerate(lens):
        t[b, n:] = 0
    return t


def _train_call(qkv, up, p, masks, form, n_valid=None, lengths=None):
    """forward and backward -> out, lse, dqkv on the CPU"""
    from pnpp_hip import transformer as T
    qg = qkv.clone().cuda().requires_grad_(True)
    out, lse = T.attention(qg, H, want_lse=True, p=p, masks=masks, n_valid=n_valid, lengths=lengths, form=form)
    (out * up.cuda()).sum().backward()
    return out.detach().cpu(), lse.cpu(), qg.grad.cpu()


@functools.lru_cache(maxsize=None)
def _reference64(p):
    """float64 attention of every cloud alone and unpadded, with the same keep bits: computed once, shared by the forms"""
    qkv, up = _inputs()
    masks = _masks(p)
    keep = _unpack(masks[0], N) if masks is not None else None
    return [_attention64(qkv[b:b + 1, :n], H, up[b:b + 1, :n], None if keep is None else keep[b:b + 1, :, :n, :n], p) for b, n in enumerate(LENS)]


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("form", FORMS)
def test_attention_ragged_against_uniform(form, p):
    """Per cloud: out[:len], lse[:len] and the whole of dqkv bit-equal to the existing call on that cloud alone with n_valid = len
    (its d_out padding rows zero, as that call's contract asks; the ragged call is handed a d_out that is random there too);
    rows >= len of out and dqkv exact zeros, lse 0 there; nothing changes when the padding rows of qkv are refilled; and the values
    are float64's under ATT_GATE."""
    qkv, up = _inputs()
    masks = _masks(p)
    lengths = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    out, lse, dqkv = _train_call(qkv, up, p, masks, form, lengths=lengths)
    up0 = _zero_padding(up, LENS)
    for b, n in enumerate(LENS):
        mb = None if masks is None else (masks[0][b:b + 1].contiguous(), masks[1][b:b + 1].contiguous())
        o1, l1, g1 = _train_call(qkv[b:b + 1], up0[b:b + 1], p, mb, form, n_valid=n)
        assert torch.equal(out[b, :n], o1[0, :n]), (form, p, b, n, "out")
        assert torch.equal(lse[b, :, :n], l1[0, :, :n]), (form, p, b, n, "lse")
        assert torch.equal(dqkv[b], g1[0]), (form, p, b, n, "dqkv")
        assert bool((out[b, n:] == 0).all()) and bool((dqkv[b, n:] == 0).all()) and bool((lse[b, :, n:] == 0).all()), (form, p, b, n, "padding")
    # the padding rows of qkv refilled with other finite values (and the lengths given as a list: validated on the host, uploaded)
    other = qkv.clone()
    fill = torch.randn(B, N, 3 * E, generator=torch.Generator().manual_seed(5)) * 4.0
    for b, n in enumerate(LENS):
        other[b, n:] = fill[b, n:]
    again = _train_call(other, up, p, masks, form, lengths=LENS)
    assert all(torch.equal(a, c) for a, c in zip((out, lse, dqkv), again))
    for b, (n, ref) in enumerate(zip(LENS, _reference64(p))):
        _check_attention(f"ragged {form} p{p} cloud {b} len {n}", (out[b:b + 1], lse[b:b + 1], dqkv[b:b + 1]), ref, n)


def test_attention_infer_ragged_against_uniform():
    """pnpp_attention_infer_ragged: the same properties for the forward-only kernel (no lse, no mask)"""
    from pnpp_hip import _lib as L
    from pnpp_hip import ops
    lib = L.lib()
    qkv, _ = _inputs()
    q = qkv.cuda()
    lengths = torch.tensor(LENS, dtype=torch.int32, device="cuda")

    def ragged(t):
        out = torch.full((B, N, E), float("nan"), device="cuda")
        L.check(lib.pnpp_attention_infer_ragged(t.data_ptr(), B, N, N, lengths.data_ptr(), H, 16, out.data_ptr(), ops._stream()))
        return out.cpu()

    out = ragged(q)
    for b, n in enumerate(LENS):
        one, o1 = q[b:b + 1].contiguous(), torch.empty(1, N, E, device="cuda")
        L.check(lib.pnpp_attention_infer(one.data_ptr(), 1, N, n, H, 16, o1.data_ptr(), ops._stream()))
        assert torch.equal(out[b, :n], o1.cpu()[0, :n]), (b, n)
        assert bool((out[b, n:] == 0).all()), (b, n)
    other = qkv.clone()
    for b, n in enumerate(LENS):
        other[b, n:] = 7.5
    assert torch.equal(ragged(other.cuda()), out)
    for b, (n, ref) in enumerate(zip(LENS, _reference64(0.0))):
        e = _maxerr(out[b:b + 1, :n], ref[0])
        assert e <= ATT_GATE * max(1.0, float(ref[0].abs().max())), (b, n, e)


def test_mean_points_ragged():
    """float64 under the gates of test_mean_points_bands (1e-6 for y, 2^-22 relative for dx); padding rows of dx exact zeros; the
    padded buffer is read in place (its padding rows hold NaN)"""
    from pnpp_hip import transformer as T
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, N, E, generator=g)
    up = torch.randn(B, E, generator=g)
    poisoned = x.clone()
    for b, n in enumerate(LENS):
        poisoned[b, n:] = float("nan")
    xg = poisoned.cuda().requires_grad_(True)
    y = T.mean_points(xg, LENS)
    (y * up.cuda()).sum().backward()
    dx = xg.grad.cpu()
    for b, n in enumerate(LENS):
        e_y = _maxerr(y[b], x[b, :n].double().mean(0))
        gref = (up[b].double() / n)[None, :].expand(n, E)
        gerr = (dx[b, :n].double() - gref).abs()
        print(f"[mean_points ragged len {n}] y {e_y:.2e} (gate 1.00e-06)  dx worst relative {float((gerr / gref.abs().clamp_min(1e-300)).max()):.2e}")
        assert e_y <= 1e-6, (b, n, e_y)
        assert bool((gerr <= 2.0 ** -22 * gref.abs()).all()), (b, n)
        assert bool((dx[b, n:] == 0).all()), (b, n)


# ------------------------------------------------------------------------------------------------ model level
@functools.lru_cache(maxsize=None)
def _clouds():
    g = torch.Generator().manual_seed(300)
    return torch.randn(B, N_PTS, 3, generator=g), torch.randn(B, 3, generator=g)


def _with_padding(x, value):
    x = x.clone()
    for b, n in enumerate(MODEL_LENS):
        x[b, n:] = value
    return x


def _stock64(m64, x):
    """the model's own containers in float64 on each cloud alone and unpadded: input_proj -> transformer -> mean -> fc_out"""
    return torch.cat([m64.fc_out(m64.transformer(m64.input_proj(x[b:b + 1, :n].double())).mean(1)) for b, n in enumerate(MODEL_LENS)])


def test_model_eval_ragged():
    x, _ = _clouds()
    model = _pt_model()
    m64 = copy.deepcopy(model).double().eval()
    with torch.no_grad():
        ref = _stock64(m64, x)
    model = model.cuda().eval()
    with torch.no_grad():
        out = model(_with_padding(x, 3.0).cuda(), MODEL_LENS)
        nan = model(_with_padding(x, float("nan")).cuda(), torch.tensor(MODEL_LENS, dtype=torch.int32, device="cuda"))
        zero = model(_with_padding(x, 0.0).cuda(), torch.tensor(MODEL_LENS))
    err, gate = _maxerr(out, ref), 2e-5 * max(1.0, float(ref.abs().max()))
    print(f"\n[PT ragged eval, {B} clouds in {N_PTS} rows] |out - float64| {err:.2e} (gate {gate:.2e})")
    assert err <= gate, err
    assert torch.equal(nan, out) and torch.equal(zero, out)


@pytest.mark.parametrize("form", FORMS)
def test_training_step_ragged(form):
    """train mode, dropout 0, MSE loss against float64 autograd of the per-cloud evaluations; then one step at the default dropout"""
    from pnpp_hip import ops
    x, tgt = _clouds()
    model = _pt_model()
    model.set_dropout(0.0)
    m64 = copy.deepcopy(model).double().train()
    ref = _stock64(m64, x)
    l64 = ((ref - tgt.double()) ** 2).mean()
    l64.backward()
    model = model.cuda().train().set_attention(form)
    out = model(_with_padding(x, float("nan")).cuda(), MODEL_LENS)
    loss = ops.mse_loss(out, tgt.cuda())
    loss.backward()
    scale = max(1.0, float(ref.detach().abs().max()))
    e_out, e_loss = _maxerr(out, ref), abs(loss.item() - float(l64.detach()))
    worst, r64 = 0.0, dict(m64.named_parameters())
    for name, p in model.named_parameters():
        r = r64[name].grad
        worst = max(worst, float((p.grad.detach().cpu().double() - r).norm() / r.norm().clamp_min(1e-30)))
    print(f"\n[PT ragged train, {form}] out {e_out:.2e} (gate {2e-5 * scale:.2e})  loss {e_loss:.2e} (gate {1e-5 * max(1.0, float(l64.detach())):.2e})  "
          f"worst per-tensor gradient relL2 {worst:.2e} (gate 1e-03)")
    assert e_out <= 2e-5 * scale
    assert e_loss <= 1e-5 * max(1.0, float(l64.detach()))
    assert worst <= 1e-3, worst
    model.set_dropout(0.1)                                    # one step with the default dropout runs and is finite
    model.zero_grad()
    loss = ops.mse_loss(model(x.cuda(), MODEL_LENS), tgt.cuda())
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())


@pytest.mark.parametrize("attention", ["split", "float32"])
def test_predictor_ragged(attention):
    """The fused kernels with lengths: all stages fused, float64's values, and -- the finite-rows invariant -- the same bits after
    every reusable buffer has been filled with NaN"""
    from pnpp_hip.inference import Predictor
    x, _ = _clouds()
    model = _pt_model()
    m64 = copy.deepcopy(model).double().eval()
    with torch.no_grad():
        ref = _stock64(m64, x)
    model = model.cuda().eval()
    pred = Predictor(model, attention=attention)
    xin = _with_padding(x, float("nan")).cuda()
    out = pred(xin, MODEL_LENS)
    assert set(pred.last_plan.values()) == {"fused"}, pred.last_plan
    assert pred.last_attention == attention
    with torch.no_grad():
        ev = model(xin, MODEL_LENS)
    err, gate = _maxerr(out, ref), 2e-5 * max(1.0, float(ref.abs().max()))
    print(f"\n[PT ragged Predictor, {attention}] |out - float64| {err:.2e} (gate {gate:.2e})   |out - model.eval()| {_maxerr(out, ev):.2e}")
    assert err <= gate, err
    tags = set()
    for (tag, _, _), t in pred._bufs.items():
        if tag in ("x", "qkv", "attention", "partial"):
            (t.view(torch.float32) if t.dtype == torch.uint8 else t).fill_(float("nan"))
            tags.add(tag)
    assert tags == {"x", "qkv", "attention", "partial"}
    assert torch.equal(pred(xin, MODEL_LENS), out)


def test_uniform_lengths_are_the_call_without_lengths():
    """lengths = [n_pts] * B: bit-equal to the call without lengths -- the model in eval mode, the gradients at dropout 0 in both
    attention forms, and the Predictor in both of its forms"""
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    x, tgt = _clouds()
    xg, tg, full = x.cuda(), tgt.cuda(), [N_PTS] * B
    model = _pt_model().cuda().eval()
    with torch.no_grad():
        assert torch.equal(model(xg, full), model(xg))
    for attention in ("split", "float32"):
        pred = Predictor(model, attention=attention)
        assert torch.equal(pred(xg, full), pred(xg)), attention
    model.train().set_dropout(0.0)
    for form in FORMS:
        model.set_attention(form)
        grads = []
        for lengths in (None, full):
            model.zero_grad()
            ops.mse_loss(model(xg, lengths), tg).backward()
            grads.append([p.grad.clone() for p in model.parameters()])
        assert all(torch.equal(a, c) for a, c in zip(*grads)), form
