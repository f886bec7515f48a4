"""Ragged batches of the vanilla PointNet (models/pointnet.py) through `lengths`: the packed-row kernels of csrc/pointnet_kernels.hip
and the ragged form of the fused inference trunk (csrc/pointnet_infer_kernels.hip).

The float64 oracle is plain torch kept in this file: pack the valid rows, linear layers, BatchNorm over the packed rows, each
cloud's max by a loop.  It shares nothing with the code under test.  Gates are those of tests/test_gpu_pointnet.py: 1e-6 for the
transforms, 1e-5 for the pooled layer with the kernel's routes handed to the oracle (ops.pn_pool_tap), 1e-4 at model level (the
oracle takes its own max there), 5e-5 absolute for the eval-mode per-cloud equivalence.

The pooled layer takes packed rows, which have no padding of their own; its cases therefore start from a padded (B, N, 128) input
that two pass-through ops.pn_transform calls pack, so that "padding is never read" and "the gradient at padding is an exact zero"
are checked through the layer as well."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LENS5 = (320, 1, 63, 64, 257)          # padded N = 320: four Gram slices of 96 rows, clouds shorter than one slice, both sides of
POOL_SHAPES = {"five": (5, 320, LENS5), "eight": (2, 1056, (1056, 129))}   # the 32- and 64-row tile edges; N = 1056: eight slices
LENS6 = (256, 33, 64, 65, 1, 200)
LENS6_EVAL = (256, 33, 64, 65, 200, 97)


def relmax(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _pack(x, lens):
    """(B, N, ...) -> the valid rows, cloud after cloud"""
    return torch.cat([x[b, :n] for b, n in enumerate(lens)], 0)


def _poison(x, lens, value, dim=1):
    """a copy of x with `value` at the padding positions along `dim`"""
    x = x.clone()
    for b, n in enumerate(lens):
        x[b].narrow(dim - 1, n, x.shape[dim] - n).fill_(value)
    return x


def _padding_is(x, lens, value, dim=1):
    return all(bool((x[b].narrow(dim - 1, n, x.shape[dim] - n) == value).all()) for b, n in enumerate(lens))


def _same(a, b):
    """bit-equal and free of NaN"""
    return all(torch.equal(a[k], b[k]) and not bool(torch.isnan(a[k]).any()) for k in a) and a.keys() == b.keys()


# ------------------------------------------------------------------------------------------------ 1. the pooled layer
@functools.lru_cache(maxsize=None)
def _pool_run(shape, training, relu, pad):
    import torch.nn as nn
    from pnpp_hip import ops
    B, N, lens = POOL_SHAPES[shape]
    K, C = 128, 128
    torch.manual_seed(5)
    conv, bn = nn.Conv1d(K, C, 1), nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C))                     # a good share of gamma < 0: those channels pool the minimum of z
        bn.bias.copy_(torch.randn(C) * 0.5)
        bn.running_mean.copy_(torch.randn(C) * 0.1)
        bn.running_var.copy_(torch.rand(C) + 0.5)
    a0 = torch.randn(B, N, K) + 0.3
    up = torch.randn(B, C)
    init = {"rm": bn.running_mean.clone(), "rv": bn.running_var.clone(), "a0": a0, "up": up,
            "w": conv.weight.detach().view(C, K).clone(), "b": conv.bias.detach().clone(), "g": bn.weight.detach().clone(),
            "be": bn.bias.detach().clone()}
    conv, bn = conv.cuda(), bn.cuda()
    ap = _poison(a0, lens, pad)
    xa, xb = ap[..., :64].contiguous().cuda().requires_grad_(True), ap[..., 64:].contiguous().cuda().requires_grad_(True)
    ops.pn_pool_tap = []
    try:
        rows = torch.cat([ops.pn_transform(xa, None, 64, lengths=list(lens)), ops.pn_transform(xb, None, 64, lengths=list(lens))], 1)
        out = ops.pn_pool(rows, B, N, conv, bn, relu, training, lengths=list(lens))
        route = ops.pn_pool_tap[0]["route"].cpu().clone()
    finally:
        ops.pn_pool_tap = None
    (out * up.cuda()).sum().backward()
    got = {"out": out.detach(), "da": torch.cat([xa.grad, xb.grad], 2), "dw": conv.weight.grad.view(C, K), "db": conv.bias.grad,
           "dg": bn.weight.grad, "dbe": bn.bias.grad, "rm": bn.running_mean, "rv": bn.running_var,
           "nbt": bn.num_batches_tracked.float(), "route": route.float()}
    return {k: v.detach().cpu().clone() for k, v in got.items()}, init


@pytest.mark.parametrize("shape", ["five", "eight"])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
def test_pooled_layer_vs_float64(shape, training, relu):
    B, N, lens = POOL_SHAPES[shape]
    got, init = _pool_run(shape, training, relu, 0.0)
    M, C = sum(lens), 128
    P = {k: init[k].double().requires_grad_(True) for k in ("w", "b", "g", "be")}
    ad = _pack(init["a0"], lens).double().requires_grad_(True)
    z = ad @ P["w"].t() + P["b"]
    if training:
        mu, var = z.mean(0), z.var(0, unbiased=False)       # over the M valid rows, each counted once
    else:
        mu, var = init["rm"].double(), init["rv"].double()
    y = (z - mu) / torch.sqrt(var + 1e-5) * P["g"] + P["be"]
    if relu:
        y = torch.relu(y)
    route = got["route"].long()
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    for b, n in enumerate(lens):
        assert int(route[b].min()) >= 0 and int(route[b].max()) < n, b      # cloud-local rows, never a padding row
    ref = torch.stack([y[offs[b]:offs[b + 1]].gather(0, route[b].unsqueeze(0)).squeeze(0) for b in range(B)])
    (ref * init["up"].double()).sum().backward()
    # the routes are each cloud's extreme of the float64 z over its own rows (up to near-ties)
    zd = z.detach()
    sel = torch.stack([zd[offs[b]:offs[b + 1]].gather(0, route[b].unsqueeze(0)).squeeze(0) for b in range(B)])
    ext = torch.stack([torch.where(P["g"].detach() >= 0, zd[offs[b]:offs[b + 1]].max(0).values, zd[offs[b]:offs[b + 1]].min(0).values)
                       for b in range(B)])
    assert float((sel - ext).abs().max()) < 1e-4
    assert relmax(got["out"], ref) < 1e-5
    assert relmax(_pack(got["da"], lens), ad.grad) < 1e-5
    assert _padding_is(got["da"], lens, 0.0)
    assert relmax(got["dw"], P["w"].grad) < 1e-5
    assert relmax(got["dg"], P["g"].grad) < 1e-5
    assert relmax(got["dbe"], P["be"].grad) < 1e-5
    if training:
        assert float(got["db"].abs().max()) == 0.0
        assert relmax(got["rm"], 0.9 * init["rm"].double() + 0.1 * mu.detach()) < 1e-6
        assert relmax(got["rv"], 0.9 * init["rv"].double() + 0.1 * var.detach() * M / (M - 1)) < 1e-6
        assert int(got["nbt"]) == 1
    else:
        assert relmax(got["db"], P["b"].grad) < 1e-5
        assert torch.equal(got["rm"], init["rm"]) and torch.equal(got["rv"], init["rv"])


# ------------------------------------------------------------------------------------------------ 2. the transforms
@functools.lru_cache(maxsize=None)
def _transform_run(D, k, layout, pad):
    from pnpp_hip import ops
    B, N, lens = 5, 320, LENS5
    g = torch.Generator().manual_seed(D * 1000 + N)
    x0 = torch.randn(B, N, D, generator=g)
    t0 = torch.randn(B, k, k, generator=g) / k ** 0.5
    ldy = ((D + 3) // 4) * 4
    up = torch.randn(sum(lens), ldy, generator=g)
    xp = _poison(x0, lens, pad)
    if layout == "bdn":
        xg = xp.transpose(1, 2).contiguous().cuda().requires_grad_(True)   # (B, D, N) storage, read through the transpose
        xin = xg.transpose(1, 2)
    else:
        xg = xp.cuda().requires_grad_(True)
        xin = xg
    tg = t0.cuda().requires_grad_(True)
    y = ops.pn_transform(xin, tg, ldy, lengths=list(lens))
    (y * up.cuda()).sum().backward()
    dx = xg.grad.transpose(1, 2) if layout == "bdn" else xg.grad
    got = {"y": y.detach().cpu().clone(), "dx": dx.detach().cpu().clone(), "dt": tg.grad.detach().cpu().clone()}
    return got, (x0, t0, up, ldy)


@pytest.mark.parametrize("D,k", [(3, 3), (64, 64)])
@pytest.mark.parametrize("layout", ["bdn", "bnd"])
def test_transform_forward_backward(D, k, layout):
    lens = LENS5
    got, (x0, t0, up, ldy) = _transform_run(D, k, layout, 0.0)
    xd, td = x0.double().requires_grad_(True), t0.double().requires_grad_(True)
    yd = torch.cat([torch.cat([xd[b, :n, :k] @ td[b], xd[b, :n, k:], xd.new_zeros(n, ldy - D)], 1) for b, n in enumerate(lens)], 0)
    (yd * up.double()).sum().backward()
    assert got["y"].shape == (sum(lens), ldy)
    assert relmax(got["y"], yd) < 1e-6
    assert relmax(got["dx"], xd.grad) < 1e-6
    assert _padding_is(got["dx"], lens, 0.0)                 # exactly 0.0 at padding
    assert relmax(got["dt"], td.grad) < 1e-6


def test_transform_of_packed_rows():
    """the feature transform's form: the input is an already packed layer"""
    from pnpp_hip import ops
    B, N, lens = 5, 320, LENS5
    g = torch.Generator().manual_seed(77)
    x0 = torch.randn(sum(lens), 64, generator=g)
    t0 = torch.randn(B, 64, 64, generator=g) / 8
    up = torch.randn(sum(lens), 64, generator=g)
    xg, tg = x0.cuda().requires_grad_(True), t0.cuda().requires_grad_(True)
    y = ops.pn_transform(xg, tg, 64, lengths=list(lens), B=B, N=N)
    (y * up.cuda()).sum().backward()
    xd, td = x0.double().requires_grad_(True), t0.double().requires_grad_(True)
    o, parts = 0, []
    for b, n in enumerate(lens):
        parts.append(xd[o:o + n] @ td[b])
        o += n
    yd = torch.cat(parts, 0)
    (yd * up.double()).sum().backward()
    assert relmax(y, yd) < 1e-6 and relmax(xg.grad, xd.grad) < 1e-6 and relmax(tg.grad, td.grad) < 1e-6


# ------------------------------------------------------------------------------------------------ the model and its float64 oracle
def _bn64(P, pre, z, train, stats):
    if train:
        mu, var = z.mean(0), z.var(0, unbiased=False)
        if stats is not None:
            stats[pre] = (mu.detach(), var.detach(), z.shape[0])
    else:
        mu, var = P[pre + ".running_mean"], P[pre + ".running_var"]
    return (z - mu) / torch.sqrt(var + 1e-5) * P[pre + ".weight"] + P[pre + ".bias"]


def _lin64(P, pre, h):
    w = P[pre + ".weight"]
    return h @ w.view(w.shape[0], -1).t() + P[pre + ".bias"]


def _cloud_max(y, lens, routes=None):
    """each cloud's max over its own rows; routes (an iterator of (B, C) cloud-local rows, in call order): the values at those rows"""
    r = None if routes is None else next(routes).long()
    o, rows = 0, []
    for b, n in enumerate(lens):
        rows.append(y[o:o + n].max(0).values if r is None else y[o:o + n].gather(0, r[b].unsqueeze(0)).squeeze(0))
        o += n
    return torch.stack(rows)


def _cloud_matmul(rows, lens, T):
    o, parts = 0, []
    for b, n in enumerate(lens):
        parts.append(rows[o:o + n] @ T[b])
        o += n
    return torch.cat(parts, 0)


def _tnet64(P, pre, rows, lens, k, train, stats, routes=None):
    h = torch.relu(_bn64(P, pre + ".bn1", _lin64(P, pre + ".conv1", rows), train, stats))
    h = torch.relu(_bn64(P, pre + ".bn2", _lin64(P, pre + ".conv2", h), train, stats))
    g = _cloud_max(torch.relu(_bn64(P, pre + ".bn3", _lin64(P, pre + ".conv3", h), train, stats)), lens, routes)
    g = torch.relu(_bn64(P, pre + ".bn4", _lin64(P, pre + ".fc1", g), train, stats))
    g = torch.relu(_bn64(P, pre + ".bn5", _lin64(P, pre + ".fc2", g), train, stats))
    return (_lin64(P, pre + ".fc3", g) + torch.eye(k, dtype=g.dtype).flatten()).view(len(lens), k, k)


def _encoder64(P, pre, x, lens, train, feature_transform, global_feat, stats=None, routes=None):
    """x (B, N, D) float64, cloud b its first lens[b] rows -> the reference network on the concatenation of the valid points"""
    routes = None if routes is None else iter(routes)
    B, N, D = x.shape
    rows = _pack(x, lens)
    trans = _tnet64(P, pre + "stn", rows, lens, 3, train, stats, routes)
    y = torch.cat([_cloud_matmul(rows[:, :3], lens, trans), rows[:, 3:]], 1)
    h = torch.relu(_bn64(P, pre + "bn1", _lin64(P, pre + "conv1", y), train, stats))
    tf = None
    if feature_transform:
        tf = _tnet64(P, pre + "fstn", h, lens, 64, train, stats, routes)
        h = _cloud_matmul(h, lens, tf)
    pf = h
    h = torch.relu(_bn64(P, pre + "bn2", _lin64(P, pre + "conv2", h), train, stats))
    g = _cloud_max(_bn64(P, pre + "bn3", _lin64(P, pre + "conv3", h), train, stats), lens, routes)
    if global_feat:
        return g, trans, tf
    o, cols = 0, []
    for b, n in enumerate(lens):
        blk = torch.cat([g[b].unsqueeze(1).expand(1024, n), pf[o:o + n].t()], 0)
        cols.append(torch.cat([blk, blk.new_zeros(1088, N - n)], 1))
        o += n
    return torch.stack(cols), trans, tf


def _pointnet64(P, x, lens, mask, train, feature_transform, stats=None):
    g, trans, tf = _encoder64(P, "encoder.", x, lens, train, feature_transform, True, stats)
    h = torch.relu(_bn64(P, "bn1", _lin64(P, "fc1", g), train, stats))
    h = _lin64(P, "fc2", h)
    if train:
        h = h * mask / 0.6
    h = torch.relu(_bn64(P, "bn2", h, train, stats))
    return _lin64(P, "fc3", h), trans, tf


def _reg64(tf):
    k = tf.shape[1]
    return (torch.bmm(tf, tf.transpose(1, 2)) - torch.eye(k, dtype=tf.dtype)).flatten(1).norm(dim=1).mean()


def _params64(state):
    return {k: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() else v.cpu()) for k, v in state.items()}


def _loss(out, t, tf):
    from pnpp_hip import ops
    loss = ops.mse_rows(out, t).mean()
    return loss if tf is None else loss + 0.001 * ops.feature_transform_regularizer(tf)


def _model_data(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 3, generator=g)
    t = torch.randn(B, 3, generator=g)
    mask = (torch.rand(B, 256, generator=g) < 0.6).to(torch.uint8)
    return x, t, mask


def _step(model, x, t, mask, lens):
    """one training step's forward and backward -> everything it produced, on the CPU"""
    xg = x.cuda().requires_grad_(True)
    kw = {} if lens is None else {"lengths": lens if isinstance(lens, torch.Tensor) else list(lens)}
    out, trans, tf = model(xg, drop_mask=mask.cuda(), return_transforms=True, **kw)
    loss = _loss(out, t.cuda(), tf)
    loss.backward()
    got = {"out": out, "trans": trans, "loss": loss, "dx": xg.grad}
    if tf is not None:
        got["trans_feat"] = tf
    for n, p in model.named_parameters():
        got["grad." + n] = p.grad
    for n, b in model.named_buffers():
        got["buf." + n] = b.float()
    return {k: v.detach().cpu().clone() for k, v in got.items()}


# ------------------------------------------------------------------------------------------------ 3. padding is never read
@pytest.mark.parametrize("shape", ["five", "eight"])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
def test_pooled_layer_never_reads_padding(shape, training, relu):
    clean, nan = _pool_run(shape, training, relu, 0.0)[0], _pool_run(shape, training, relu, float("nan"))[0]
    assert _same(clean, nan)


@pytest.mark.parametrize("D,k", [(3, 3), (64, 64)])
@pytest.mark.parametrize("layout", ["bdn", "bnd"])
def test_transform_never_reads_padding(D, k, layout):
    assert _same(_transform_run(D, k, layout, 0.0)[0], _transform_run(D, k, layout, float("nan"))[0])


def test_pointnet_step_never_reads_padding():
    from models.pointnet import PointNet
    B, N, lens = 6, 256, LENS6
    torch.manual_seed(11)
    m0 = PointNet(True).cuda().train()
    x, t, mask = _model_data(B, N, 21)
    runs = [_step(copy.deepcopy(m0), _poison(x, lens, pad), t, mask, lens) for pad in (0.0, float("nan"))]
    assert _same(runs[0], runs[1])
    assert _padding_is(runs[1]["dx"], lens, 0.0)


# ------------------------------------------------------------------------------------------------ 4. lengths == N is the uniform call
def test_full_lengths_equal_the_uniform_call_bitwise():
    from models.pointnet import PointNet
    B, N = 4, 256
    torch.manual_seed(11)
    m0 = PointNet(feature_transform=True).cuda().train()
    x, t, mask = _model_data(B, N, 31)
    uni = _step(copy.deepcopy(m0), x, t, mask, None)
    rag = _step(copy.deepcopy(m0), x, t, mask, (N,) * B)
    assert uni.keys() == rag.keys() and "trans_feat" in uni
    for k in uni:
        assert torch.equal(uni[k], rag[k]), k


# ------------------------------------------------------------------------------------------------ 5. the model against float64
def _model_vs_float64(feature_transform, lens, B, N):
    from models.pointnet import PointNet
    torch.manual_seed(11)
    m = PointNet(feature_transform)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda().train()
    x, t, mask = _model_data(B, N, B + N)
    got = _step(m, _poison(x, lens, float("nan")) if lens is not None else x, t, mask, lens)
    P = _params64(state)
    stats = {}
    o64, tr64, tf64 = _pointnet64(P, x.double(), lens if lens is not None else (N,) * B, mask.double(), True, feature_transform, stats)
    l64 = ((o64 - t.double()) ** 2).mean()
    if feature_transform:
        l64 = l64 + 0.001 * _reg64(tf64)
    l64.backward()
    err = {"out": relmax(got["out"], o64), "trans": relmax(got["trans"], tr64),
           "loss": abs(float(got["loss"]) - float(l64.detach())) / abs(float(l64.detach()))}
    if feature_transform:
        err["trans_feat"] = relmax(got["trans_feat"], tf64)
    names = [n for n, _ in m.named_parameters()]
    g = torch.cat([got["grad." + n].double().flatten() for n in names])
    r = torch.cat([P[n].grad.flatten() for n in names])
    err["grad"] = float((g - r).norm() / r.norm())
    worst = 0.0
    for pre, (mu, var, M) in stats.items():
        worst = max(worst, relmax(got["buf." + pre + ".running_mean"], 0.9 * state[pre + ".running_mean"].double() + 0.1 * mu))
        worst = max(worst, relmax(got["buf." + pre + ".running_var"],
                                  0.9 * state[pre + ".running_var"].double() + 0.1 * var * M / (M - 1)))
    err["running"] = worst
    per_point = [p for p in stats if p.endswith(("bn1", "bn2", "bn3")) and p.startswith("encoder")]
    assert all(stats[p][2] == (sum(lens) if lens is not None else B * N) for p in per_point) and len(per_point) >= 6
    return err


@pytest.mark.parametrize("feature_transform", [True, False])
def test_pointnet_vs_float64_train(feature_transform):
    err = _model_vs_float64(feature_transform, LENS6, 6, 256)
    print(f"\n[pointnet ragged ft={feature_transform}] " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k, v in err.items():
        assert v < 1e-4, (k, v)


# ------------------------------------------------------------------------------------------------ 6. eval: each cloud on its own
@pytest.fixture(scope="module")
def eval_model():
    from models.pointnet import PointNet
    torch.manual_seed(2)
    m = PointNet(True).cuda().train()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        m(torch.randn(8, 128, 3, generator=g).cuda())        # one train-mode pass: running statistics move off their init
    return m.eval()


def test_eval_rows_equal_the_per_cloud_calls(eval_model):
    from pnpp_hip.inference import Predictor
    m, B, N, lens = eval_model, 6, 256, LENS6_EVAL
    x = _poison(_model_data(B, N, 41)[0], lens, float("nan")).transpose(1, 2).contiguous().cuda()    # (B, 3, N)
    pred = Predictor(m)
    with torch.no_grad():
        outs = {"model": m(x, return_transforms=True, lengths=list(lens)), "predictor": pred(x, return_transforms=True, lengths=list(lens))}
        dev = pred(x, return_transforms=True, lengths=torch.tensor(lens, dtype=torch.int32).cuda())
        alone = [m(x[b:b + 1, :, :n].contiguous(), return_transforms=True) for b, n in enumerate(lens)]
        alone_p = [tuple(v.clone() for v in pred(x[b:b + 1, :, :n].contiguous(), return_transforms=True)) for b, n in enumerate(lens)]
    assert pred.last_plan["encoder"] == "fused"
    for a, b in zip(outs["predictor"], dev):                 # a device lengths tensor gives the same bits
        assert torch.equal(a, b)
    for who, ref in (("model", alone), ("predictor", alone_p)):
        for i in range(3):
            for b in range(B):
                d = float((outs[who][i][b] - ref[b][i][0]).abs().max())
                assert d < 5e-5, (who, i, b, d)


def test_infer_trunk_is_bitwise_the_per_cloud_launch(eval_model):
    from pnpp_hip.inference import Predictor
    from pnpp_hip.lengths import packed_lengths
    B, N, lens = 6, 256, LENS6_EVAL
    pred = Predictor(eval_model)
    xr = _poison(_model_data(B, N, 43)[0], lens, float("nan")).cuda()                               # (B, N, 3)
    pk = packed_lengths(list(lens), B, N, xr.device)
    g = torch.Generator().manual_seed(5)
    trans = (torch.eye(3) + 0.1 * torch.randn(B, 3, 3, generator=g)).cuda()
    tf = (torch.eye(64) + 0.1 * torch.randn(B, 64, 64, generator=g)).cuda()
    for name, args in (("stn", (None, None)), ("fstn", (trans, None)), ("encoder", (trans, tf))):
        want = name == "encoder"                             # the encoder trunk also taps its 64-wide rows (global_feat=False)
        out, feat = (v.clone() if v is not None else None for v in pred._trunk(name, xr, *args, want_feat=want, pk=pk))
        assert pred.last_plan[name] == "fused"
        assert not bool(torch.isnan(out).any())
        for b, n in enumerate(lens):
            a = tuple(v[b:b + 1] if v is not None else None for v in args)
            o1, f1 = pred._trunk(name, xr[b:b + 1, :n].contiguous(), *a, want_feat=want)
            assert torch.equal(out[b], o1[0]), (name, b)
            if want:
                fb = feat.view(B, N, 64)[b]
                assert torch.equal(fb[:n], f1) and bool((fb[n:] == 0).all()), (name, b)


# ------------------------------------------------------------------------------------------------ 7. global_feat=False
def test_encoder_pointwise_output_and_backward():
    """Values against the oracle's own max.  The gradient of a max jumps where two rows tie, and this loss (a random weight on every
    element of the (B, 1088, N) output) puts ~16 times the weight of a point feature on each pooled entry, so a single route that
    differs from the float64 argmax moves the flat gradient by ~2e-2: measured once, one of 18432 routes picked a row 2.7e-6 below
    the float64 maximum (float32 cannot resolve that) and the unrouted comparison read 2.1e-2 while the routed one read 5.5e-6; the
    uniform call at the same B, N and seed read 1.1e-5 either way.  The gradient comparison therefore hands the kernel's routes to
    the oracle (ops.pn_pool_tap, as for the pooled layer), after checking that each routed value is within 1e-4 of the oracle's
    own maximum; the gate stays 1e-4."""
    from models.pointnet import PointNetEncoder
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    B, N, lens = 6, 256, LENS6
    torch.manual_seed(3)
    enc = PointNetEncoder(global_feat=False, feature_transform=True, channel=6)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    enc = enc.cuda().train()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, 6, N, generator=g)
    up = torch.randn(B, 1088, N, generator=g)
    xg = _poison(x, lens, float("nan"), dim=2).cuda().requires_grad_(True)
    ops.pn_pool_tap = []
    try:
        out, trans, tf = enc(xg, lengths=list(lens))
        routes = [d["route"].cpu().clone() for d in ops.pn_pool_tap]
    finally:
        ops.pn_pool_tap = None
    assert out.shape == (B, 1088, N) and len(routes) == 3
    assert _padding_is(out.detach().cpu(), lens, 0.0, dim=2)  # exact zeros in the padding columns
    ((out * _poison(up, lens, float("nan"), dim=2).cuda()).sum() + ops.feature_transform_regularizer(tf)).backward()
    P = {"enc." + k: v for k, v in _params64(state).items()}
    with torch.no_grad():                                    # unrouted: the oracle's own max
        o64, tr64, tf64 = _encoder64(P, "enc.", x.double().transpose(1, 2), lens, True, True, False)
    assert relmax(out, o64) < 1e-4 and relmax(trans, tr64) < 1e-4 and relmax(tf, tf64) < 1e-4
    r64, tr64, tf64 = _encoder64(P, "enc.", x.double().transpose(1, 2), lens, True, True, False, routes=routes)
    assert float((r64.detach() - o64).abs().max()) < 1e-4              # the routed rows are the maxima up to near-ties
    ((r64 * up.double()).sum() + _reg64(tf64)).backward()
    names = [n for n, _ in enc.named_parameters()]
    for n in names:
        assert bool(torch.isfinite(dict(enc.named_parameters())[n].grad).all()), n
    assert bool(torch.isfinite(xg.grad).all()) and _padding_is(xg.grad.cpu(), lens, 0.0, dim=2)
    got = torch.cat([dict(enc.named_parameters())[n].grad.double().cpu().flatten() for n in names])
    ref = torch.cat([P["enc." + n].grad.flatten() for n in names])
    assert float((got - ref).norm() / ref.norm()) < 1e-4
    # the forward-only path: the same zeros, rows as the eval-mode model's
    enc.eval()
    lens_e = LENS6_EVAL
    xe = _poison(x, lens_e, float("nan"), dim=2).cuda()
    with torch.no_grad():
        ev = enc(xe, lengths=list(lens_e))[0]
        pr = Predictor(enc)(xe, lengths=list(lens_e))[0]
    assert _padding_is(pr.cpu(), lens_e, 0.0, dim=2) and _padding_is(ev.cpu(), lens_e, 0.0, dim=2)
    assert float((pr - ev).abs().max()) < 5e-5 * max(1.0, float(ev.abs().max()))


# ------------------------------------------------------------------------------------------------ 8. repeatability
def test_two_identical_ragged_steps_bitwise():
    from models.pointnet import PointNet
    B, N, lens = 6, 256, LENS6
    torch.manual_seed(5)
    m0 = PointNet(True).cuda().train()
    x, t, mask = _model_data(B, N, 51)
    a, b = (_step(copy.deepcopy(m0), x, t, mask, lens) for _ in range(2))
    assert _same(a, b)
    # the lengths as a device tensor (offsets by pnpp_pn_offsets, the row count read back once): the same step
    assert _same(a, _step(copy.deepcopy(m0), x, t, mask, torch.tensor(lens, dtype=torch.int32).cuda()))


def test_ragged_predictor_call_is_capturable(eval_model):
    """Static shapes, the lengths read on the device: one captured call serves other lengths written into the same tensor."""
    from pnpp_hip.inference import Predictor
    B, N = 6, 256
    pred = Predictor(eval_model)
    x = _model_data(B, N, 61)[0].cuda()
    lens_dev = torch.tensor(LENS6_EVAL, dtype=torch.int32).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pred(x, return_transforms=True, lengths=lens_dev)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = pred(x, return_transforms=True, lengths=lens_dev)
    for lens in (LENS6_EVAL, LENS6, (N,) * B):
        lens_dev.copy_(torch.tensor(lens, dtype=torch.int32))
        g.replay()
        eager = pred(x, return_transforms=True, lengths=list(lens))
        for a, b in zip(out, eager):
            assert torch.equal(a, b), lens
