"""Float64 parity of the point transformer's TRAINING kernels (csrc/transformer_kernels.hip) across their shape bands and edges.

tests/test_gpu_pt.py reaches each kernel at one or two shapes, the attention only with n_valid = N.  Every case below compares a HIP
result with a float64 evaluation of the same operation on the CPU, under the gates of tests/test_gpu_pt.py and
tests/test_gpu_head_loss.py, and prints its worst error beside the gate.

  attention forward, dQ, dK/dV (T.attention)   predicate crossed
    n_valid 1, 31, 32, 33                      nkbv == 1; the partial last key block ((kb + 1) * 32 > Nv) and its absence at 32
    n_valid 127, 129, 161, 257                 a 128-row workgroup whose last row only is padding / with one valid query and key; the
                                               partial query block of the dK/dV kernel; kvalid; mask words at pitch N/32, nkbv walked
    H 1, 2, 4, 8; B 1, 2, 3                    row pitch 48 .. 384, grid.y, grid.z
    p 0, 0.25                                  keep bits and padding together, by value
    padding rows 0 / 1e4                       nothing a valid row receives depends on the padding; padded rows of dqkv are zero
    rising / first-block maximum               alpha < 1 in every key block, alpha = 1 after the first
  attention_dropout_mask                       bit for bit against oracle/sampler.py: p 0 .. 0.999, stream ids beyond 2^32, device counter
  add_layernorm, forward and backward          E 8, 64, 100, 128 (second column slot); r given or not; M % 4 != 0 (row >= M); M 63, 64, 65
                                               (a backward block of one row); 16 and 65 slabs; inputs offset by 100 x their spread
  mean_points                                  N 1, 3 (idle row lanes), E 100, 128 (second channel pass), B 65, the [:, :n_pts] slice
  linear_smallk                                K 1, 3, 6, 8 (db in slab column 8); N 1, 100, 130; no bias; M 255, 256, 257 (slab edge);
                                               M 16390 (the forward's grid-stride loop)
  fc_block without a norm                      the four projections of an encoder layer (K 64 / 128, ReLU or not, keep mask or not)
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import FLIP_MARGIN, relmax
from test_gpu_pt import _unpack
from test_gpu_pt_attention_inference import _stress_qkv

pytestmark = pytest.mark.gpu

ATT_GATE = 2e-5      # tests/test_gpu_pt.py: out and dqkv relative to max(1, max|ref|), lse absolute
LN_FWD, LN_BWD = 2e-6, 1e-5


def _maxerr(got, ref):
    return float((got.detach().cpu().double().reshape(ref.shape) - ref.detach().cpu().double()).abs().max())


def _scale(ref):
    return max(1.0, float(ref.detach().abs().max()))


# ------------------------------------------------------------------------------------------------ attention
def _attention64(qkv, H, up, keep=None, p=0.0):
    """float64 softmax attention of the UNPADDED clouds qkv (B, n, 3E), dropout as softmax * keep / (1 - p) with keep (B, H, n, n):
    (out, lse, d qkv for the upstream gradient up, scaled scores)"""
    B, n, E3 = qkv.shape
    E = E3 // 3
    qd = qkv.double().requires_grad_(True)
    q, k, v = (t.reshape(B, n, H, 16).transpose(1, 2) for t in qd.split(E, dim=-1))
    s = (q * 0.25) @ k.transpose(-1, -2)
    w = torch.softmax(s, dim=-1)
    if keep is not None:
        w = w * keep / (1.0 - p)
    out = (w @ v).transpose(1, 2).reshape(B, n, E)
    (out * up.double()).sum().backward()
    return out.detach(), torch.logsumexp(s.detach(), dim=-1), qd.grad, s.detach()


def _run_attention(qkv, up, H, p, masks, nv):
    """forward and backward on the padded layout (B, N, 3E) -> out (B, N, E), lse (B, H, N), dqkv (B, N, 3E), on the CPU"""
    from pnpp_hip import transformer as T
    qg = qkv.clone().cuda().requires_grad_(True)
    out, lse = T.attention(qg, H, want_lse=True, p=p, masks=masks, n_valid=nv)
    (out * up.cuda()).sum().backward()
    return out.detach().cpu(), lse.cpu(), qg.grad.cpu()


def _padded(valid, N):
    B, n, C = valid.shape
    full = torch.zeros(B, N, C)
    full[:, :n] = valid
    return full


def _masks(B, N, H, p):
    from pnpp_hip import transformer as T
    return T.attention_dropout_mask(B, N, H, p, "cuda", seed=11, stream_id=3) if p > 0 else None


def _check_attention(tag, got, ref, nv):
    out, lse, dqkv = got
    rout, rlse, rgrad, _ = ref
    e_out, e_lse, e_g = _maxerr(out[:, :nv], rout), _maxerr(lse[..., :nv], rlse), _maxerr(dqkv[:, :nv], rgrad)
    print(f"\n[attention {tag}] out {e_out:.2e} (gate {ATT_GATE * _scale(rout):.2e})  lse {e_lse:.2e} (gate {ATT_GATE:.2e})  "
          f"dqkv {e_g:.2e} (gate {ATT_GATE * _scale(rgrad):.2e})")
    assert e_out <= ATT_GATE * _scale(rout), (tag, e_out)
    assert e_lse <= ATT_GATE, (tag, e_lse)
    assert e_g <= ATT_GATE * _scale(rgrad), (tag, e_g)
    assert bool((dqkv[:, nv:] == 0).all()), (tag, "a padding row of dqkv is not zero")


ATT_CASES = [(1, 128, 1, 1, 0.0), (1, 128, 4, 31, 0.0), (2, 128, 4, 32, 0.0), (2, 128, 2, 33, 0.0), (2, 128, 2, 33, 0.25),
             (1, 128, 4, 127, 0.0), (2, 256, 4, 129, 0.0), (2, 256, 4, 129, 0.25), (1, 256, 8, 161, 0.0), (1, 256, 8, 161, 0.25),
             (3, 384, 4, 257, 0.0), (1, 384, 1, 384, 0.25)]


def _att_inputs(B, H, nv, seed):
    g = torch.Generator().manual_seed(seed)
    E = 16 * H
    qkv = torch.randn(B, nv, 3 * E, generator=g) * 1.5
    qkv[0, :, :E] *= 3.0                                      # a cloud with peaked softmax rows
    return qkv, torch.randn(B, nv, E, generator=g)


@pytest.mark.parametrize("B,N,H,nv,p", ATT_CASES)
def test_attention_bands(B, N, H, nv, p):
    """Forward, dQ and dK/dV on a padded layout against float64 on the unpadded clouds; padded rows of dqkv exactly zero (dK/dV are
    written as zeros, dQ is exp(.) * (0 - 0)); a second call gives the same bits (no atomics)."""
    qkv, up = _att_inputs(B, H, nv, 1000 * N + nv)
    masks = _masks(B, N, H, p)
    keep = _unpack(masks[0], N)[:, :, :nv, :nv] if masks is not None else None
    ref = _attention64(qkv, H, up, keep, p)
    if nv == 1:                                               # one key: out = v, lse = the score
        assert torch.equal(ref[0], qkv[..., 2 * 16 * H:].double()) and _maxerr(ref[1], ref[3][..., 0]) == 0.0
    got = _run_attention(_padded(qkv, N), _padded(up, N), H, p, masks, nv)
    _check_attention(f"B{B} N{N} H{H} nv{nv} p{p}", got, ref, nv)
    again = _run_attention(_padded(qkv, N), _padded(up, N), H, p, masks, nv)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_attention_is_independent_of_the_padding(p):
    """The padding rows of qkv at zero, then at 1e4 (the value tests/test_gpu_pt_attention_inference.py uses): what the valid rows
    receive is the same bit for bit, everything is finite, and the padded rows of dqkv are zero.  While the dK/dV epilogue multiplied
    by kvalid = 0 instead of selecting, all 24,320 dK/dV elements of the padded rows were NaN here (P of a padded key overflows)."""
    B, N, H, nv = 2, 256, 4, 161
    qkv, up = _att_inputs(B, H, nv, 5)
    masks = _masks(B, N, H, p)
    zero = _run_attention(_padded(qkv, N), _padded(up, N), H, p, masks, nv)
    big = _padded(qkv, N)
    big[:, nv:] = 1e4
    large = _run_attention(big, _padded(up, N), H, p, masks, nv)
    nonfinite = [int((~torch.isfinite(t)).sum()) for t in large]
    print(f"\n[attention padding at 1e4, p {p}] non-finite elements of out / lse / dqkv: {nonfinite}; of them in valid rows: "
          f"{[int((~torch.isfinite(t[:, :nv] if i != 1 else t[..., :nv])).sum()) for i, t in enumerate(large)]}")
    assert nonfinite == [0, 0, 0], nonfinite
    assert torch.equal(large[0][:, :nv], zero[0][:, :nv])
    assert torch.equal(large[1][..., :nv], zero[1][..., :nv])
    assert torch.equal(large[2][:, :nv], zero[2][:, :nv])
    assert bool((large[2][:, nv:] == 0).all()) and bool((zero[2][:, nv:] == 0).all())


@pytest.mark.parametrize("first", [False, True], ids=["rising-maximum", "maximum-in-first-block"])
def test_attention_rescale_stress(first):
    """The synthetic cloud of tests/test_gpu_pt_attention_inference.py (n = 160, five key blocks) through the training kernels, padded
    to N = 256: the running maximum of every query rises in each key block (alpha < 1 four times) or sits in the first one.  Scaled
    scores within +-10: their float32 rounding is about 1e-6, a twentieth of the gate."""
    H, n, N = 4, 160, 256
    qkv = _stress_qkv(first)
    up = torch.randn(1, n, 16 * H, generator=torch.Generator().manual_seed(78))
    ref = _attention64(qkv, H, up)
    s = ref[3]
    assert float(s.abs().max()) <= 10.0, float(s.abs().max())
    bm = s.reshape(1, H, n, 5, 32).max(dim=-1).values         # per query, the maximum of each key block
    assert bool((bm[..., 0:1] > bm[..., 1:]).all()) if first else bool((bm[..., 1:] > bm[..., :-1]).all())
    got = _run_attention(_padded(qkv, N), _padded(up, N), H, 0.0, None, n)
    _check_attention("rescale stress, " + ("maximum in the first block" if first else "maximum rising in every block"), got, ref, n)
    assert all(bool(torch.isfinite(t).all()) for t in got)


@pytest.mark.parametrize("B,N,H,p,sid", [(1, 128, 1, 0.1, 3), (3, 128, 1, 0.5, (3 << 40) + 17), (2, 256, 4, 0.0, 1), (1, 384, 8, 0.999, 2),
                                         (1, 128, 2, 0.3, None)])
def test_dropout_mask_bits_match_the_restatement(B, N, H, p, sid):
    """Both orientations of the keep bits, bit for bit, against the numpy Philox restatement (oracle/sampler.py); sid None is the
    device-counter form, whose stream id is 1 + the draws made so far on this device."""
    from oracle import sampler as S
    from pnpp_hip import transformer as T
    if sid is None:
        cnt = T._att_counter(torch.device("cuda"))
        want = 1 + int(cnt[0])
        mask, maskT = T.attention_dropout_mask(B, N, H, p, "cuda", seed=11)
        assert int(cnt[0]) == want
    else:
        want = sid
        mask, maskT = T.attention_dropout_mask(B, N, H, p, "cuda", seed=11, stream_id=sid)
    rm, rmT = S.attention_dropout_mask(11, want, B, N, H, p)
    got, gotT = (t.cpu().numpy().view(np.uint32) for t in (mask, maskT))
    print(f"\n[dropout mask B{B} N{N} H{H} p{p} id {want}] differing words: mask {int((got != rm).sum())}, maskT {int((gotT != rmT).sum())}; "
          f"keep rate {float(_unpack(mask, N).mean()):.4f}")
    assert np.array_equal(got, rm) and np.array_equal(gotT, rmT)


# ------------------------------------------------------------------------------------------------ add_layernorm
@pytest.mark.parametrize("M,E,has_r,offset", [(1, 64, True, 0), (3, 128, True, 0), (5, 100, False, 0), (63, 128, True, 0), (64, 128, True, 0),
                                              (65, 128, True, 0), (1001, 64, False, 100), (4097, 128, True, 0), (7, 8, True, 0)])
def test_add_layernorm_bands(M, E, has_r, offset):
    """y, du for both addends, d weight, d bias.  The kernel adds x + r in float32, as the reference model does: the forward reference
    is float64 LayerNorm of that float32 sum (tests/test_gpu_pt.py's reference)."""
    from pnpp_hip import transformer as T
    g = torch.Generator().manual_seed(131 * M + E)
    x = 3.0 * (torch.randn(M, E, generator=g) + float(offset)) + (0.0 if offset else 1.0)
    r = torch.randn(M, E, generator=g) if has_r else None
    up = torch.randn(M, E, generator=g)
    ln = nn.LayerNorm(E)
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.5 * torch.randn(E, generator=g))
        ln.bias.copy_(0.3 * torch.randn(E, generator=g))
        ln.weight[0], ln.weight[1] = 0.0, -0.7
    assert int((ln.weight < 0).sum()) > 0 and int((ln.weight == 0).sum()) == 1
    wd, bd = (t.detach().clone().double().requires_grad_(True) for t in (ln.weight, ln.bias))
    with torch.no_grad():
        ref = nn.functional.layer_norm((x + r if has_r else x).double(), (E,), wd, bd, ln.eps)
    xd = x.double().requires_grad_(True)
    rd = r.double().requires_grad_(True) if has_r else None
    (nn.functional.layer_norm(xd + rd if has_r else xd, (E,), wd, bd, ln.eps) * up.double()).sum().backward()
    ln = ln.cuda()
    xg = x.clone().cuda().requires_grad_(True)
    rg = r.clone().cuda().requires_grad_(True) if has_r else None
    y = T.add_layernorm(xg, rg, ln)
    (y * up.cuda()).sum().backward()
    e_y = _maxerr(y, ref)
    pairs = [("dx", xg.grad, xd.grad), ("dw", ln.weight.grad, wd.grad), ("db", ln.bias.grad, bd.grad)]
    if has_r:
        pairs.insert(1, ("dr", rg.grad, rd.grad))
    errs = {n: (_maxerr(a, b), LN_BWD * _scale(b)) for n, a, b in pairs}
    print(f"\n[add_layernorm M{M} E{E} r={has_r} offset {offset}] y {e_y:.2e} (gate {LN_FWD * _scale(ref):.2e})  " +
          "  ".join(f"{n} {e:.2e} (gate {gt:.2e})" for n, (e, gt) in errs.items()))
    assert e_y <= LN_FWD * _scale(ref), e_y
    for n, (e, gt) in errs.items():
        assert e <= gt, (n, e, gt)


# ------------------------------------------------------------------------------------------------ mean_points
@pytest.mark.parametrize("B,N,E,rows", [(1, 1, 64, None), (2, 3, 64, None), (3, 5, 128, None), (2, 777, 128, None), (65, 130, 64, None),
                                        (1, 4097, 100, None), (3, 200, 64, 256)])
def test_mean_points_bands(B, N, E, rows):
    """rows: the input is the slice [:, :N] of a (B, rows, E) tensor, as the model feeds it for a padded cloud; the gradient comes back
    in the slice's shape, so the rest of the tensor's gradient is zero.  Backward: dy * (1.f / N) is two float32 roundings."""
    from pnpp_hip import transformer as T
    g = torch.Generator().manual_seed(7 * N + E)
    full = torch.randn(B, rows or N, E, generator=g)
    up = torch.randn(B, E, generator=g)
    fg = full.clone().cuda().requires_grad_(True)
    xin = fg[:, :N] if rows else fg
    assert xin.is_contiguous() == (rows is None)
    y = T.mean_points(xin)
    (y * up.cuda()).sum().backward()
    ref = full[:, :N].double().mean(1)
    gref = (up.double() / N)[:, None, :].expand(B, N, E)
    e_y = _maxerr(y, ref)
    gerr = (fg.grad[:, :N].cpu().double() - gref).abs()
    worst = float((gerr / gref.abs().clamp_min(1e-300)).max())
    print(f"\n[mean_points B{B} N{N} E{E} rows {rows}] y {e_y:.2e} (gate 1.00e-06)  dx worst relative {worst:.2e} (gate {2.0 ** -22:.2e})")
    assert y.shape == (B, E) and fg.grad.shape == full.shape
    assert e_y <= 1e-6, e_y
    assert bool((gerr <= 2.0 ** -22 * gref.abs()).all()), worst
    if rows:
        assert bool((fg.grad[:, N:] == 0).all())


# ------------------------------------------------------------------------------------------------ linear_smallk
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("M,K,N", [(1, 1, 1), (3, 3, 64), (5, 8, 64), (255, 3, 130), (256, 3, 130), (257, 3, 130), (1000, 6, 100),
                                   (16390, 3, 64)])
def test_linear_smallk_bands(M, K, N, bias):
    from pnpp_hip import transformer as T
    torch.manual_seed(M + 10 * K + N)
    lin = nn.Linear(K, N, bias=bias)
    g = torch.Generator().manual_seed(M * 3 + K)
    x, up = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    ref = x.double() @ lin.weight.detach().double().t() + (lin.bias.detach().double() if bias else 0.0)
    lin = lin.cuda()
    y = T.linear_smallk(x.cuda(), lin)
    (y * up.cuda()).sum().backward()
    e_y, e_w = _maxerr(y, ref), _maxerr(lin.weight.grad, up.double().t() @ x.double())
    e_b = _maxerr(lin.bias.grad, up.double().sum(0)) if bias else 0.0
    print(f"\n[linear_smallk M{M} K{K} N{N} bias={bias}] y {e_y:.2e} (gate {1e-6 * _scale(ref):.2e})  dW {e_w:.2e}  db {e_b:.2e} "
          f"(gate {1e-5 * M ** 0.5:.2e})")
    assert y.shape == (M, N)
    assert e_y <= 1e-6 * _scale(ref), e_y
    assert e_w <= 1e-5 * M ** 0.5 and e_b <= 1e-5 * M ** 0.5, (e_w, e_b)


# ------------------------------------------------------------------------------------------------ fc_block without a norm
@pytest.mark.parametrize("M", [384, 4224])
@pytest.mark.parametrize("K,N,relu,masked", [(64, 192, False, False), (64, 64, False, True), (64, 128, True, True), (128, 64, False, True)],
                         ids=["in_proj", "out_proj", "linear1", "linear2"])
def test_fc_block_projection_shapes(M, K, N, relu, masked):
    """The projections of an encoder layer (in_proj; out_proj, linear1 + ReLU and linear2 with their keep masks, here injected at keep
    0.9) against float64 autograd, under test_fc_block's gates.  With a ReLU the float64 evaluation takes the HIP path's decisions
    where an element is kept (a dropped element has neither value nor gradient); each differing decision sits within FLIP_MARGIN."""
    from pnpp_hip import ops
    torch.manual_seed(M + K + 3 * N)
    lin = nn.Linear(K, N)
    g = torch.Generator().manual_seed(M + N)
    x, up = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    keep = (torch.rand(M, N, generator=g) < 0.9) if masked else None
    xd = x.double().requires_grad_(True)
    W, b = (t.detach().clone().double().requires_grad_(True) for t in (lin.weight, lin.bias))
    lin = lin.cuda()
    xg = x.clone().cuda().requires_grad_(True)
    y = ops.fc_block(xg, lin, relu=relu, dropout=nn.Dropout(0.1) if masked else None, training=True,
                     mask=keep.to(torch.uint8).cuda() if masked else None)
    y.backward(up.cuda())
    z = xd @ W.t() + b
    flips = 0
    if relu:
        on = z.detach() > 0
        hip_on = torch.where(keep, y.detach().cpu() > 0, on) if masked else y.detach().cpu() > 0
        flip = hip_on != on
        flips = int(flip.sum())
        margin = float((z.detach().abs() * flip).max() / z.detach().abs().max())
        assert margin <= FLIP_MARGIN, (flips, margin)
        z = z * hip_on.double()
    y64 = z * keep.double() / 0.9 if masked else z
    (y64 * up.double()).sum().backward()
    err = {"y": relmax(y, y64), "dx": relmax(xg.grad, xd.grad), "dW": relmax(lin.weight.grad, W.grad), "db": relmax(lin.bias.grad, b.grad)}
    print(f"\n[fc_block M{M} K{K} N{N} relu={relu} mask={masked}] flips {flips}  " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()) +
          "  (gates 1e-05 / 2e-05)")
    assert err["y"] < 1e-5, err
    for k in ("dx", "dW", "db"):
        assert err[k] < 2e-5, err
