"""Float64 parity of the vanilla PointNet kernels (csrc/pointnet_kernels.hip) across their shape bands and edges.

tests/test_gpu_pointnet.py checks each kernel at one or two shapes.  The kernels branch on more than those shapes reach; every case
below compares a HIP result with a float64 evaluation of the same operation, the HIP path's discrete decisions (max routes, ReLU
masks) injected, each output under its own gate, and the kernels a band must reach asserted through tests/dispatch.py.

  pooled wide layer (ops.pn_pool)    predicate crossed
    N  1 .. 4096                     pn_gram_slices: 1 / 4 / 8 row slices at N = 256 / 1024; 32-row Gram steps, 64-row scan / dA tiles
    B  1 .. 1000                     the per-lane cloud loops of pn_pool_finalize / pn_pool_bwd_channels (b = lane; b < B; b += 64)
    K  4, 8, 64, 68, 124, 128        one or two 64-wide Gram tiles, a partial second tile, K % 8 != 0 in pn_pool_bwd_da
    C  64, 128, 960, 1024            one channel block, pn_pool_bwd_q's 32-channel staging, a full PN_CMAX route list
    offset inputs                    dA's BatchNorm-statistics part for columns whose mean is many times their spread
  fc_block, BatchNorm + ReLU         fc_backward's row-chunked BatchNorm pair for M > 4096 (fc_bwd_bn_rows_sums / _apply)
  pn_bn_relu, pn_concat, pn_add_identity, the regulariser, pn_transform at their block and tile edges
  PointNet                           pn_trunk's M > 32 floor, the head's M <= 32 paths left, M = 4096, 8 Gram slices; per-tensor gates
"""
import ctypes

import pytest
import torch
import torch.nn as nn

from conftest import FLIP_MARGIN, ROUTE_GAP
from dispatch import expect, field, find, record
from test_gpu_pointnet import _ReluDecisions, _params64, _reg64, _run_model, pointnet_ref, relmax

pytestmark = pytest.mark.gpu

GATE = 1e-5          # per tensor, relative to its own max-abs: kernel level
MODEL_GATE = 1e-4    # per tensor, model level


def _dev64(work):
    """Where the float64 evaluation runs: on the GPU once it is large (work = B*N*C multiply-adds per input column)."""
    return "cuda" if work > 2_000_000 else "cpu"


def _slices(N):
    """Row slices per cloud of the Gram launch, restated from DESIGN section 10 (pn_gram_slices)."""
    return 8 if N >= 1024 else 4 if N >= 256 else 1


# ------------------------------------------------------------------------------------------------ pooled wide layer
def _pool_layer(K, C, seed, training):
    torch.manual_seed(seed)
    conv, bn = nn.Conv1d(K, C, 1), nn.BatchNorm1d(C)
    with torch.no_grad():
        g = torch.randn(C)
        g[torch.randperm(C)[:3]] = 0.0          # a_c = 0 takes the max branch
        bn.weight.copy_(g)
        bn.bias.copy_(torch.randn(C) * 0.5)
        bn.running_mean.copy_(torch.randn(C) * 0.1)
        bn.running_var.copy_(torch.rand(C) + 0.5)
    assert int((bn.weight < 0).sum()) > 0 and int((bn.weight == 0).sum()) == 3
    return conv, bn


def _pool_input(B, N, K, gen, dup=None, offset=0.0):
    if offset:
        std = torch.rand(K, generator=gen) * 1.5 + 0.5
        sign = torch.where(torch.rand(K, generator=gen) < 0.5, -1.0, 1.0)
        a = (sign * offset * std + std * torch.randn(B * N, K, generator=gen)).view(B, N, K)
    else:
        a = (torch.randn(B * N, K, generator=gen) + 0.3).view(B, N, K)
    if dup == "row":                             # row 1 large (an extremum of many channels), copied to the last row of its cloud
        a[:, 1] *= 5.0
        a[:, N - 1] = a[:, 1]
    elif dup == "cloud":                         # cloud 0: N identical rows; cloud 1 normal, so the statistics stay defined
        a[0] = a[0, 0]
    return a.reshape(B * N, K).contiguous()


def _check_pool(B, N, K, C, training, relu, dup=None, offset=0.0, want_da=True, seed=0, z_gate=GATE):
    """One pn_pool forward + backward against float64; returns {part: error}.  z_gate bounds the output and dgamma, the parts that
    read z at the route, whose float32 rounding grows with the inputs' offset (everything else: GATE)."""
    from pnpp_hip import ops
    from test_gpu_pointnet import _pool_ref
    conv, bn = _pool_layer(K, C, seed + B * 7 + N * 13 + K * 17 + C, training)
    a0 = _pool_input(B, N, K, torch.Generator().manual_seed(seed + N), dup, offset)
    up = torch.randn(B, C, generator=torch.Generator().manual_seed(seed + 1))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    conv, bn = conv.cuda(), bn.cuda()
    ag = a0.cuda().requires_grad_(want_da)
    ops.pn_pool_tap = []
    res = {}

    def run():
        res["out"] = ops.pn_pool(ag, B, N, conv, bn, relu, training)
        (res["out"] * up.cuda()).sum().backward()

    try:
        tags = record(run)
        tap = ops.pn_pool_tap[0]
    finally:
        ops.pn_pool_tap = None
    out = res["out"]
    # the kernels this case must have run
    gram = ["pn_gram_kernel", "pn_gram_reduce_kernel", "pn_pool_bwd_q_kernel"]
    expect(tags, present=["pn_pool_scan_kernel", "pn_pool_finalize_kernel", "pn_pool_bwd_channels_kernel"] + (gram if training else []),
           absent=([] if training else gram) + ([] if want_da else ["pn_pool_bwd_da_kernel", "pn_pool_bwd_q_kernel"]))
    if want_da:
        expect(tags, present=["pn_pool_bwd_da_kernel"])
    if training:
        (g,) = find(tags, "pn_gram_kernel")
        assert field(g, "slices") == _slices(N), g
    assert int(bn.num_batches_tracked) == int(training)

    dev = _dev64(B * N * C)
    P = {n: p.detach().to(dev).double().requires_grad_(True) for n, p in
         (("w", conv.weight.view(C, K)), ("b", conv.bias), ("g", bn.weight), ("be", bn.bias))}
    ad = a0.to(dev).double().requires_grad_(True)
    route = tap["route"].to(dev).long()
    assert int(route.min()) >= 0 and int(route.max()) < N
    ref, mu, var = _pool_ref(ad, P["w"], P["b"], P["g"], P["be"], route, B, N, relu, training,
                             rm0.double().to(dev), rv0.double().to(dev))
    (ref * up.double().to(dev)).sum().backward()

    # routes: float32 rounding away from float64's own extremum; ties resolve to the lowest row
    zd = (ad @ P["w"].t() + P["b"]).detach().view(B, N, C)
    sel = zd.gather(1, route.unsqueeze(1)).squeeze(1)
    ext = torch.where(P["g"].detach() >= 0, zd.max(1).values, zd.min(1).values)   # a_c = 0 takes the max
    res["route_gap"] = float(((sel - ext).abs() / ext.abs().clamp_min(1.0)).max())
    assert res["route_gap"] <= ROUTE_GAP, res["route_gap"]
    if dup == "row" and N > 2:
        assert int((route == N - 1).sum()) == 0, "a tie between rows 1 and N-1 went to the later row"
        assert int((route == 1).sum()) > B * C // 10, "the duplicated row is an extremum of too few channels to test the tie"
    if dup == "cloud":
        assert int(route[0].abs().max()) == 0, "a cloud of identical rows must route every channel to its first row"

    res["out_err"] = relmax(out, ref)
    res["dw"] = relmax(conv.weight.grad.view(C, K), P["w"].grad)
    res["dgamma"] = relmax(bn.weight.grad, P["g"].grad)
    res["dbeta"] = relmax(bn.bias.grad, P["be"].grad)
    if not training:
        res["db"] = relmax(conv.bias.grad, P["b"].grad)
    if want_da:
        routed = torch.zeros(B, N, dtype=torch.bool, device=dev)
        routed.scatter_(1, route, True)
        routed = routed.view(B * N)
        dag, dad = ag.grad.to(dev).double(), ad.grad
        res["da_routed"] = relmax(dag[routed], dad[routed])
        if training and bool((~routed).any()):
            res["da_rest"] = relmax(dag[~routed], dad[~routed])
        if not training and bool((~routed).any()):
            assert float(dag[~routed].abs().max()) == 0.0, "eval mode: rows no route reaches get no gradient"
    else:
        assert ag.grad is None
    print(f"\n[pn_pool B{B} N{N} K{K} C{C} {'train' if training else 'eval'}{' offset %g' % offset if offset else ''}] " +
          " ".join(f"{k} {v:.1e}" for k, v in res.items() if isinstance(v, float)))
    for k, v in res.items():
        if isinstance(v, float) and k != "route_gap":
            assert v < (z_gate if k in ("out_err", "dgamma") else GATE), (k, v)
    if training:
        assert float(conv.bias.grad.abs().max()) == 0.0
        M = B * N
        assert relmax(bn.running_mean, 0.9 * rm0.double() + 0.1 * mu.detach().cpu()) < 1e-6
        assert relmax(bn.running_var, 0.9 * rv0.double() + 0.1 * var.detach().cpu() * M / (M - 1)) < 1e-6
    else:
        assert torch.equal(bn.running_mean.cpu(), rm0) and torch.equal(bn.running_var.cpu(), rv0)
    return res


# (B, N, K, C, training, relu, extra): every N, B, K and C of the bands, training / eval, relu on / off, both tie kinds
POOL_CASES = [
    (2, 1, 128, 1024, False, True, {}),          # one row per cloud; full route list
    (65, 1, 64, 128, True, False, {}),           # N = 1 in training (M = 65); second lane iteration
    (63, 2, 8, 64, True, True, {}),
    (1, 31, 4, 64, False, False, {"want_da": False}),
    (1, 1023, 68, 128, True, True, {}),          # B = 1; 4 slices; partial second Gram tile
    (2, 63, 124, 960, True, False, {}),          # K % 8 = 4; 15 channel blocks
    (64, 64, 128, 256, True, True, {}),
    (2, 65, 68, 64, False, True, {}),
    (2, 255, 64, 128, True, True, {}),           # last N with one slice
    (2, 256, 128, 64, True, False, {}),          # first N with four
    (2, 257, 4, 1024, True, True, {}),
    (2, 1024, 8, 128, True, False, {}),          # first N with eight
    (2, 1025, 124, 64, True, True, {}),
    (2, 2500, 128, 1024, True, True, {}),
    (1, 4096, 64, 256, False, False, {}),
    (2, 4096, 128, 128, True, False, {}),
    (130, 31, 128, 128, True, True, {}),         # three lane iterations
    (1000, 3, 128, 64, True, True, {}),          # sixteen
    (65, 100, 68, 960, False, True, {}),
    (4, 300, 128, 256, True, True, {"dup": "row"}),
    (3, 65, 8, 64, False, True, {"dup": "row"}),
    (2, 64, 64, 128, True, False, {"dup": "cloud"}),
    (2, 100, 128, 1024, False, False, {"dup": "cloud"}),
]


@pytest.mark.parametrize("B,N,K,C,training,relu,extra", POOL_CASES,
                         ids=[f"B{c[0]}-N{c[1]}-K{c[2]}-C{c[3]}-{'train' if c[4] else 'eval'}-{'relu' if c[5] else 'id'}"
                              + (f"-{c[6]['dup']}" if "dup" in c[6] else "") for c in POOL_CASES])
def test_pooled_layer_bands(B, N, K, C, training, relu, extra):
    _check_pool(B, N, K, C, training, relu, **extra)


@pytest.mark.parametrize("offset", [0, 3, 30, 100])
@pytest.mark.parametrize("B,N,K,C,relu", [(4, 300, 128, 256, True), (32, 1024, 128, 1024, False)])
def test_pooled_layer_offset_inputs(B, N, K, C, relu, offset):
    """Columns of A with mean = offset x std (a post-BN-ReLU channel after training): the rows no route reaches carry only the
    BatchNorm-statistics part of dA, Q (A_n - S/M) - W^T(a o g), which must not lose digits to the offset (it lost them before
    pn_pool_bwd_da centred its tile: 1.3e-5 at offset 30).  The output and dgamma read the float32 z = A W^T + b of the routed row,
    rounded at the scale of |A|, not of its spread: ~1.5e-7 per unit of offset, held to GATE x offset / 30."""
    _check_pool(B, N, K, C, True, relu, offset=float(offset), seed=3, z_gate=GATE * max(1.0, offset / 30))


# ------------------------------------------------------------------------------------------------ fc_block at the trunks' shapes
def _fc_layer(K, N, seed, pad):
    torch.manual_seed(seed)
    lin, bn = nn.Linear(K, N), nn.BatchNorm1d(N)
    with torch.no_grad():
        if pad:                                  # the first layers read (x, y, z, 0) rows with a zero-padded weight column
            lin.weight[:, 3:] = 0.0
        bn.weight.copy_(torch.randn(N))
        bn.bias.copy_(torch.rand(N) - 0.5)
        bn.running_mean.copy_(torch.randn(N) * 0.1)
        bn.running_var.copy_(torch.rand(N) + 0.5)
    return lin, bn


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("K,N", [(4, 64), (64, 64), (64, 128)])
@pytest.mark.parametrize("M", [33, 4096, 4097, 5000, 32768])
def test_fc_block_trunk_shapes(M, K, N, training):
    from pnpp_hip import ops
    lin, bn = _fc_layer(K, N, M + K + N, K == 4)
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g)
    if K == 4:
        x[:, 3] = 0.0
    up = torch.randn(M, N, generator=g)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    lin, bn = lin.cuda(), bn.cuda()
    xg = x.cuda().requires_grad_(True)
    res = {}

    def run():
        with _ReluDecisions() as rd:
            res["y"] = ops.fc_block(xg, lin, bn, relu=True, training=training)
        res["mask"] = rd.masks[0]
        res["y"].backward(up.cuda())

    tags = record(run)
    rows = ["fc_bwd_bn_rows_sums_kernel", "fc_bwd_bn_rows_apply_kernel"]
    expect(tags, present=rows if M > 4096 else [], absent=[] if M > 4096 else rows)

    dev = _dev64(M * N * 8)
    xd = x.to(dev).double().requires_grad_(True)
    W, b = (p.detach().to(dev).double().requires_grad_(True) for p in (lin.weight, lin.bias))
    gm, bt = (p.detach().to(dev).double().requires_grad_(True) for p in (bn.weight, bn.bias))
    z = xd @ W.t() + b
    mu, var = (z.mean(0), z.var(0, unbiased=False)) if training else (rm0.double().to(dev), rv0.double().to(dev))
    yl = (z - mu) / torch.sqrt(var + bn.eps) * gm + bt
    mask = res["mask"].to(dev)
    flip = mask != (yl.detach() > 0)
    margin = float((yl.detach().abs() * flip).max() / yl.detach().abs().max()) if bool(flip.any()) else 0.0
    assert margin <= FLIP_MARGIN, (int(flip.sum()), margin)
    y64 = yl * mask.double()
    (y64 * up.to(dev).double()).sum().backward()
    err = {"y": relmax(res["y"], y64), "dx": relmax(xg.grad, xd.grad), "dw": relmax(lin.weight.grad, W.grad),
           "dgamma": relmax(bn.weight.grad, gm.grad), "dbeta": relmax(bn.bias.grad, bt.grad)}
    print(f"\n[fc_block M{M} K{K} N{N} {'train' if training else 'eval'}] flips {int(flip.sum())} " +
          " ".join(f"{k} {v:.1e}" for k, v in err.items()))
    assert err["y"] < GATE, err
    for k in ("dx", "dw", "dgamma", "dbeta"):
        assert err[k] < 2 * GATE, err
    if training:
        assert float(lin.bias.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) < 1e-9
        assert relmax(bn.running_mean, 0.9 * rm0.double() + 0.1 * mu.detach().cpu()) < GATE
        assert relmax(bn.running_var, 0.9 * rv0.double() + 0.1 * var.detach().cpu() * M / (M - 1)) < GATE
    else:
        assert relmax(lin.bias.grad, b.grad) < 2 * GATE
        assert torch.equal(bn.running_mean.cpu(), rm0) and torch.equal(bn.running_var.cpu(), rv0)


@pytest.mark.parametrize("training", [True, False])
def test_fc_recompute_output_same_bits(training):
    """pnpp_fc_recompute_output, called the way _PnTrunk calls it, gives the forward pass's y bit for bit."""
    from pnpp_hip import _lib as L
    from pnpp_hip import ops
    lib = L.lib()
    for M in (33, 4096, 4097):
        for K, N in ((4, 64), (64, 64), (64, 128)):
            lin, bn = _fc_layer(K, N, M * 3 + N, K == 4)
            lin, bn = lin.cuda(), bn.cuda()
            x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + K)).cuda()
            d = L.FcDesc()
            d.M, d.K, d.N, d.norm, d.relu, d.training = M, K, N, L.NORM_BATCH, 1, int(training)
            d.eps, d.momentum, d.drop_scale = bn.eps, 0.1, 1.0
            saved = torch.empty(lib.pnpp_fc_saved_bytes(ctypes.byref(d)), dtype=torch.uint8, device="cuda")
            scratch = ops._scratch(lib.pnpp_fc_scratch_bytes(ctypes.byref(d)), x.device)
            y = torch.full((M, N), float("nan"), device="cuda")
            a = L.FcFwdArgs()
            a.x, a.w, a.b = x.data_ptr(), lin.weight.data_ptr(), lin.bias.data_ptr()
            a.nw, a.nb, a.rm, a.rv = bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr()
            a.y, a.saved, a.scratch = y.data_ptr(), saved.data_ptr(), scratch.data_ptr()
            L.check(lib.pnpp_fc_forward(ctypes.byref(d), ctypes.byref(a), ops._stream()))
            y2 = torch.full((M, N), float("nan"), device="cuda")
            L.check(lib.pnpp_fc_recompute_output(ctypes.byref(d), saved.data_ptr(), None, y2.data_ptr(), ops._stream()))
            assert bool(torch.isfinite(y).all()) and float((y > 0).float().mean()) > 0.2
            assert torch.equal(y, y2), (M, K, N)


# ------------------------------------------------------------------------------------------------ the small kernels
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("C", [256, 257, 512])
@pytest.mark.parametrize("M", [2, 3, 32, 33, 300])
def test_bn_relu_bands(M, C, training):
    """ops.pn_bn_relu against float64 BatchNorm + ReLU: channel 0 all dead, channel 1 constant (variance 0) with beta 0 (y = 0 exactly
    in training), channel 2 with mean exactly 0, zeros among its values and beta 0 (y = 0 exactly at those rows)."""
    from pnpp_hip import ops
    g = torch.Generator().manual_seed(M * 1000 + C)
    bn = nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g))
        bn.bias.copy_(torch.rand(C, generator=g) - 0.5)
        bn.weight[0], bn.bias[0] = 0.1, -10.0
        bn.bias[1] = bn.bias[2] = 0.0
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        bn.running_mean[2] = 0.0
    x = torch.randn(M, C, generator=g) + 0.2
    x[:, 1] = 0.7
    h = (M - 1) // 2
    x[:, 2] = 0.0
    x[:h, 2], x[h:2 * h, 2] = 1.0, -1.0
    up = torch.randn(M, C, generator=g)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn = bn.cuda()
    xg = x.cuda().requires_grad_(True)
    y = ops.pn_bn_relu(xg, bn, training)
    (y * up.cuda()).sum().backward()
    xd = x.double().requires_grad_(True)
    gm, bt = bn.weight.detach().cpu().double().requires_grad_(True), bn.bias.detach().cpu().double().requires_grad_(True)
    mu, var = (xd.mean(0), xd.var(0, unbiased=False)) if training else (rm0.double(), rv0.double())
    yl = (xd - mu) / torch.sqrt(var + bn.eps) * gm + bt
    mask = (y.detach() > 0).cpu()
    flip = mask != (yl.detach() > 0)
    assert not bool(flip.any()) or float((yl.detach().abs() * flip).max() / yl.detach().abs().max()) <= FLIP_MARGIN
    y64 = yl * mask.double()
    (y64 * up.double()).sum().backward()
    assert float(y[:, 0].abs().max()) == 0.0 and float(xg.grad[:, 0].abs().max()) == 0.0
    if training:
        assert float(y[:, 1].abs().max()) == 0.0
    if M >= 3:
        assert float(y[(x[:, 2] == 0).cuda(), 2].abs().max()) == 0.0
    err = {"y": relmax(y, y64), "dgamma": relmax(bn.weight.grad, gm.grad), "dbeta": relmax(bn.bias.grad, bt.grad)}
    if training and M == 2:
        # two rows: x_hat = +-sqrt(var / (var + eps)), so dx = gamma istd (h_n - mean h)(1 - x_hat^2) = O(eps / var) of its terms;
        # float32 can only be held to the scale of those terms here
        scale = (gm.detach() * torch.rsqrt(var.detach() + bn.eps) * up.double() * mask.double()).abs().max()
        err["dx"] = float((xg.grad.cpu().double() - xd.grad).abs().max() / scale)
    else:
        err["dx"] = relmax(xg.grad, xd.grad)
    for k, v in err.items():
        assert v < GATE, (k, err)
    if training:
        assert int(bn.num_batches_tracked) == 1
        assert relmax(bn.running_mean, 0.9 * rm0.double() + 0.1 * mu.detach()) < 1e-6
        assert relmax(bn.running_var, 0.9 * rv0.double() + 0.1 * var.detach() * M / (M - 1)) < 1e-6
    else:
        assert torch.equal(bn.running_mean.cpu(), rm0) and torch.equal(bn.running_var.cpu(), rv0)


def test_bn_relu_training_refuses_one_row():
    from pnpp_hip import ops
    bn = nn.BatchNorm1d(256).cuda()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.pn_bn_relu(torch.randn(1, 256, device="cuda"), bn, True)
    y = ops.pn_bn_relu(torch.randn(1, 256, device="cuda"), bn, False)      # eval mode takes one row
    assert y.shape == (1, 256)


@pytest.mark.parametrize("C1,C2", [(4, 1), (1024, 64)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 65, 1000])
def test_concat_bands(N, B, C1, C2):
    from pnpp_hip import ops
    g = torch.Generator().manual_seed(N + B + C1)
    gf, pf, up = torch.randn(B, C1, generator=g), torch.randn(B * N, C2, generator=g), torch.randn(B, C1 + C2, N, generator=g)
    gg, pg = gf.cuda().requires_grad_(True), pf.cuda().requires_grad_(True)
    out = ops.pn_concat(gg, pg, N)
    ref = torch.cat([gf.unsqueeze(2).expand(B, C1, N), pf.view(B, N, C2).transpose(1, 2)], 1)
    assert torch.equal(out.cpu(), ref)
    out.backward(up.cuda())
    assert relmax(gg.grad, up.double()[:, :C1].sum(2)) < 1e-6
    assert torch.equal(pg.grad.cpu(), up[:, C1:].transpose(1, 2).reshape(B * N, C2))


@pytest.mark.parametrize("k,B", [(1, 1), (1, 70), (3, 5), (3, 70), (64, 1), (64, 70)])
def test_add_identity_bands(k, B):
    from pnpp_hip import ops
    x = torch.randn(B, k * k, generator=torch.Generator().manual_seed(k * 100 + B))
    xg = x.cuda().requires_grad_(True)
    y = ops.pn_add_identity(xg, k)
    assert torch.equal(y.cpu(), x.view(B, k, k) + torch.eye(k))
    up = torch.randn(B, k, k)
    y.backward(up.cuda())
    assert torch.equal(xg.grad.cpu(), up.view(B, k * k))


@pytest.mark.parametrize("k", [1, 2, 3, 17, 64])
@pytest.mark.parametrize("B", [1, 65])
def test_regularizer_bands(B, k):
    """The last cloud's T is a permutation matrix: its norm is 0 and so is its gradient (torch's norm backward and the kernel's
    nb > 0 guard).  With B = 1 that is the whole batch: the value and every gradient are exactly 0."""
    from pnpp_hip import ops
    g = torch.Generator().manual_seed(k * 10 + B)
    t0 = torch.eye(k) + 0.3 * torch.randn(B, k, k, generator=g)
    t0[-1] = torch.eye(k)[torch.randperm(k, generator=g)]
    td = t0.double().requires_grad_(True)
    ref = _reg64(td)
    (ref * 0.7).backward()
    assert float(td.grad[-1].abs().max()) == 0.0
    tg = t0.cuda().requires_grad_(True)
    r = ops.feature_transform_regularizer(tg)
    (r * 0.7).backward()
    assert r.shape == () and abs(float(r.detach()) - float(ref.detach())) <= 1e-6 * float(ref)
    assert float(tg.grad[-1].abs().max()) == 0.0
    assert relmax(tg.grad, td.grad) < 1e-6


@pytest.mark.parametrize("layout", ["bdn", "bnd"])
@pytest.mark.parametrize("B,N,D,k,ldy", [(65, 64, 4, 1, 4), (65, 65, 1, 1, 4), (3, 65, 64, 3, 64), (3, 64, 3, 3, 64), (65, 65, 6, 3, 64)])
def test_transform_edges(B, N, D, k, ldy, layout):
    from pnpp_hip import ops
    g = torch.Generator().manual_seed(B * N + D * 10 + k)
    x0 = torch.randn(B, N, D, generator=g)
    t0 = torch.randn(B, k, k, generator=g) / k ** 0.5
    up = torch.randn(B * N, ldy, generator=g)
    xd, td = x0.double().requires_grad_(True), t0.double().requires_grad_(True)
    yd = torch.cat([torch.bmm(xd[..., :k], td), xd[..., k:], xd.new_zeros(B, N, ldy - D)], 2).reshape(B * N, ldy)
    (yd * up.double()).sum().backward()
    if layout == "bdn":
        xg = x0.transpose(1, 2).contiguous().cuda().requires_grad_(True)
        xin = xg.transpose(1, 2)
    else:
        xg = x0.cuda().requires_grad_(True)
        xin = xg
    tg = t0.cuda().requires_grad_(True)
    y = ops.pn_transform(xin, tg, ldy)
    (y * up.cuda()).sum().backward()
    assert relmax(y, yd) < 1e-6
    if ldy > D:
        assert float(y[:, D:].abs().max()) == 0.0
    dx = xg.grad.transpose(1, 2) if layout == "bdn" else xg.grad
    assert relmax(dx, xd.grad) < 1e-6
    assert relmax(tg.grad, td.grad) < 1e-6


# ------------------------------------------------------------------------------------------------ model level, per-tensor gates
def _bias_before_bn(name):
    """Biases of the layers right in front of a train-mode BatchNorm: it cancels them, zero in exact arithmetic and on the HIP path."""
    parts = name.split(".")
    return parts[-1] == "bias" and (parts[-2] in ("conv1", "conv2", "conv3") or (parts[-2] in ("fc1", "fc2") and len(parts) > 2)
                                    or name == "fc1.bias")


def _check_model_tensors(B, N, training):
    """PointNet(feature_transform=True) against the float64 restatement, routes and ReLU decisions injected.  Gates out, trans,
    trans_feat, the loss and each parameter tensor's gradient against its own max, and the flat gradient norm."""
    from models.pointnet import PointNet
    torch.manual_seed(11)
    m = PointNet(True).cuda().train()
    g = torch.Generator().manual_seed(B * 1000 + N)
    if not training:
        with torch.no_grad():
            m(torch.randn(B, N, 3, generator=g).cuda())     # running statistics move off their init
        m.eval()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, t = torch.randn(B, N, 3, generator=g), torch.randn(B, 3, generator=g)
    mask = (torch.rand(B, 256, generator=g) < 0.6).to(torch.uint8) if training else None
    relu = []
    out, loss, routes, trans, tf = _run_model(m, x.cuda(), None if mask is None else mask.cuda(), t.cuda(), relu)
    loss.backward()
    P = _params64(state, "cuda")
    P["_relu"] = iter(relu)
    o64, tr64, tf64 = pointnet_ref(P, x.double().cuda(), routes, None if mask is None else mask.double().cuda(), training, True)
    l64 = ((o64 - t.double().cuda()) ** 2).mean() + 0.001 * _reg64(tf64)
    l64.backward()
    assert len(routes) == 3
    err = {"out": relmax(out, o64), "trans": relmax(trans, tr64), "trans_feat": relmax(tf, tf64),
           "loss": abs(float(loss) - float(l64)) / abs(float(l64))}
    params = dict(m.named_parameters())
    top = max(float(P[n].grad.abs().max()) for n in params)
    for n, p in params.items():
        ref = P[n].grad
        if training and _bias_before_bn(n):
            assert float(p.grad.abs().max()) == 0.0 and float(ref.abs().max()) < 1e-9, n
        elif float(ref.abs().max()) < 1e-9 * top:
            # zero in exact arithmetic by another route (the pooled layer's beta when a linear layer and a train-mode BatchNorm
            # follow it): float32 leaves noise, held to the gate on the scale of the same BatchNorm's gamma gradient
            sib = float(P[n[:-len("bias")] + "weight"].grad.abs().max())
            assert float(p.grad.abs().max()) <= MODEL_GATE * sib, (n, float(p.grad.abs().max()), sib)
        else:
            err["d " + n] = relmax(p.grad, ref)
    names = list(params)
    got = torch.cat([params[n].grad.detach().double().flatten() for n in names])
    flat = float((got - torch.cat([P[n].grad.flatten() for n in names])).norm() / torch.cat([P[n].grad.flatten() for n in names]).norm())
    worst = max(err, key=err.get)
    print(f"\n[PointNet B{B} N{N} {'train' if training else 'eval'}] out {err['out']:.1e} trans {err['trans']:.1e} "
          f"trans_feat {err['trans_feat']:.1e} loss {err['loss']:.1e}; flat grad {flat:.1e}; worst {worst} {err[worst]:.1e} "
          f"over {sum(k.startswith('d ') for k in err)} tensors")
    bad = {k: v for k, v in err.items() if not v < MODEL_GATE}
    assert not bad, bad
    assert flat < MODEL_GATE, flat


@pytest.mark.parametrize("B,N,training", [(33, 128, True), (64, 64, True), (65, 100, False), (2, 17, False), (3, 2500, False)])
def test_pointnet_bands_per_tensor(B, N, training):
    """(33, 128): the head leaves its M <= 32 paths and the narrow layers take the row-chunked BatchNorm backward (M = 4224);
    (64, 64): M = 4096 exactly; (65, 100) eval; (2, 17): M = 34, just above pn_trunk's floor; (3, 2500): 7500 rows."""
    _check_model_tensors(B, N, training)


@pytest.mark.parametrize("B,N", [(2, 17), (3, 2500)])
def test_trunk_small_batch_training(B, N):
    """ops.pn_trunk in training with 2 or 3 clouds, a T-Net's trunk (4 -> 64 -> 128 -> pooled 1024 + ReLU): M = 34 just above the
    floor, and 8 Gram slices with partial tiles at N = 2500.  Per tensor against float64 with the routes and ReLU decisions
    injected.  The whole model is gated per tensor at these sizes in eval mode only: in training its heads normalise over the B
    clouds, and with two rows x_hat = +-1 up to eps, so float64's own output and gradients there are O(eps / var) of their terms
    (measured: the output 2e-2 apart at B = 2, 1.5e-3 at B = 3) -- a property of BatchNorm over 2 rows, not of the kernels."""
    from pnpp_hip import ops
    torch.manual_seed(B + N)
    layers = [(nn.Conv1d(4, 64, 1), nn.BatchNorm1d(64)), (nn.Conv1d(64, 128, 1), nn.BatchNorm1d(128))]
    pooled = (nn.Conv1d(128, 1024, 1), nn.BatchNorm1d(1024))
    with torch.no_grad():
        layers[0][0].weight[:, 3:] = 0.0
    mods = [m for pair in layers + [pooled] for m in pair]
    state = [(p.detach().clone().double().cuda().requires_grad_(True)) for m in mods for p in (m.weight, m.bias)]
    for m in mods:
        m.cuda()
    g = torch.Generator().manual_seed(N)
    rows = torch.randn(B * N, 4, generator=g)
    rows[:, 3] = 0.0
    up = torch.randn(B, 1024, generator=g).cuda()
    rg = rows.cuda().requires_grad_(True)
    ops.pn_pool_tap, ops.pn_relu_tap = [], []
    try:
        tags = record(lambda: (ops.pn_trunk(rg, B, N, [(c, n) for c, n in layers], pooled, True, True) * up).sum().backward())
        route, masks = ops.pn_pool_tap[0]["route"].long(), [m_.cuda() for m_ in ops.pn_relu_tap]
    finally:
        ops.pn_pool_tap, ops.pn_relu_tap = None, None
    (gk,) = find(tags, "pn_gram_kernel")
    assert field(gk, "slices") == _slices(N), gk
    expect(tags, present=["fc_bwd_bn_rows_sums_kernel"] if B * N > 4096 else [],
           absent=[] if B * N > 4096 else ["fc_bwd_bn_rows_sums_kernel"])

    def bn64(z, gm, bt):
        return (z - z.mean(0)) / torch.sqrt(z.var(0, unbiased=False) + 1e-5) * gm + bt

    h = rows.double().cuda().requires_grad_(True)
    x = h
    for li in range(2):
        w, b, gm, bt = state[4 * li:4 * li + 4]
        y = bn64(x @ w.view(w.shape[0], -1).t() + b, gm, bt)
        flip = masks[li] != (y.detach() > 0)
        assert not bool(flip.any()) or float((y.detach().abs() * flip).max() / y.detach().abs().max()) <= FLIP_MARGIN
        x = y * masks[li].double()
    w, b, gm, bt = state[8:12]
    out64 = torch.relu(bn64(x @ w.view(1024, -1).t() + b, gm, bt)).view(B, N, 1024).gather(1, route.unsqueeze(1)).squeeze(1)
    (out64 * up.double()).sum().backward()
    err = {"d rows": relmax(rg.grad, h.grad)}
    for i, (m, name) in enumerate((m, f"{j}.{k}") for j, m in enumerate(mods) for k in ("weight", "bias")):
        ref, got = state[i].grad, getattr(m, name.split(".")[1]).grad
        if isinstance(m, nn.Conv1d) and name.endswith("bias"):
            assert float(got.abs().max()) == 0.0 and float(ref.abs().max()) < 1e-9, name
            continue
        err[f"d {type(m).__name__}{name}"] = relmax(got, ref)
    worst = max(err, key=err.get)
    print(f"\n[pn_trunk B{B} N{N} train] worst {worst} {err[worst]:.1e} over {len(err)} tensors")
    bad = {k: v for k, v in err.items() if not v < MODEL_GATE}
    assert not bad, bad


@pytest.mark.parametrize("training", [True, False])
def test_pointnet_refuses_32_points_or_fewer(training):
    from models.pointnet import PointNet
    m = PointNet(True).cuda().train(training)
    with pytest.raises(ValueError, match="more than 32"):
        m(torch.randn(2, 16, 3, device="cuda"))
    torch.cuda.synchronize()
