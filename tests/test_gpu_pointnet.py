"""GPU parity of the vanilla PointNet (models/pointnet.py) and its kernels (csrc/pointnet_kernels.hip).

Kernel level: the per-cloud transform, the feature-transform regulariser and the pooled wide layer against float64 evaluations.
Model level: PointNet / PointNetEncoder against a float64 restatement kept in this file (written from the reference's module
definitions), with the HIP path's max routes of the three pooled layers injected; at the full size (32 clouds x 1024 points) also
the bytes kept for backward.  Then determinism, graph capture with the fused Adam, and a short training run."""
import copy

import pytest
import torch

from conftest import ROUTED_GATE

pytestmark = pytest.mark.gpu


def relmax(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("D,k,layout,N", [(3, 3, "bdn", 1), (3, 3, "bdn", 77), (6, 3, "bdn", 300), (6, 3, "bnd", 1000),
                                          (64, 64, "bnd", 1), (64, 64, "bnd", 130), (64, 64, "bdn", 1000)])
def test_transform_forward_backward(D, k, layout, N):
    from pnpp_hip import ops
    B = 3
    g = torch.Generator().manual_seed(D * 1000 + N)
    x0 = torch.randn(B, N, D, generator=g)
    t0 = torch.randn(B, k, k, generator=g) / k ** 0.5
    up = torch.randn(B * N, ((D + 3) // 4) * 4, generator=g)
    ldy = up.shape[1]
    xd, td = x0.double().requires_grad_(True), t0.double().requires_grad_(True)
    yd = torch.cat([torch.bmm(xd[..., :k], td), xd[..., k:], xd.new_zeros(B, N, ldy - D)], 2).reshape(B * N, ldy)
    (yd * up.double()).sum().backward()
    if layout == "bdn":
        xg = x0.transpose(1, 2).contiguous().cuda().requires_grad_(True)   # (B, D, N) storage, read through the transpose
        xin = xg.transpose(1, 2)
    else:
        xg = x0.cuda().requires_grad_(True)
        xin = xg
    tg = t0.cuda().requires_grad_(True)
    y = ops.pn_transform(xin, tg, ldy)
    (y * up.cuda()).sum().backward()
    assert relmax(y, yd) < 1e-6
    dx = xg.grad.transpose(1, 2) if layout == "bdn" else xg.grad
    assert relmax(dx, xd.grad) < 1e-6
    assert relmax(tg.grad, td.grad) < 1e-6


@pytest.mark.parametrize("k,B", [(3, 5), (64, 4)])
def test_regularizer_forward_backward(k, B):
    from pnpp_hip import ops
    g = torch.Generator().manual_seed(k)
    t0 = torch.eye(k) + 0.3 * torch.randn(B, k, k, generator=g)
    td = t0.double().requires_grad_(True)
    ref = (torch.bmm(td, td.transpose(1, 2)) - torch.eye(k, dtype=torch.float64)).flatten(1).norm(dim=1).mean()
    (ref * 0.7).backward()
    tg = t0.cuda().requires_grad_(True)
    r = ops.feature_transform_regularizer(tg)
    (r * 0.7).backward()
    assert r.shape == () and abs(float(r.detach()) - float(ref.detach())) <= 1e-6 * float(ref)
    assert relmax(tg.grad, td.grad) < 1e-6


def _pool_ref(a, w, b, gamma, beta, route, B, N, relu, training, rm=None, rv=None, eps=1e-5):
    z = a @ w.t() + b
    if training:
        mu, var = z.mean(0), z.var(0, unbiased=False)
    else:
        mu, var = rm, rv
    y = (z - mu) / torch.sqrt(var + eps) * gamma + beta
    if relu:
        y = torch.relu(y)
    return y.view(B, N, -1).gather(1, route.long().unsqueeze(1)).squeeze(1), mu, var


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
def test_pooled_wide_layer(training, relu):
    import dispatch
    import torch.nn as nn
    from pnpp_hip import ops
    B, N, K, C = 4, 300, 128, 256
    torch.manual_seed(5)
    conv, bn = nn.Conv1d(K, C, 1), nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C))                     # a good share of gamma < 0: those channels pool the minimum of z
        bn.bias.copy_(torch.randn(C) * 0.5)
        bn.running_mean.copy_(torch.randn(C) * 0.1)
        bn.running_var.copy_(torch.rand(C) + 0.5)
    assert int((bn.weight < 0).sum()) > 50
    a0 = torch.randn(B * N, K) + 0.3
    up = torch.randn(B, C)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    conv, bn = conv.cuda(), bn.cuda()
    ag = a0.cuda().requires_grad_(True)
    ops.pn_pool_tap = []
    try:
        tags = dispatch.record(lambda: ops.pn_pool(ag, B, N, conv, bn, relu, training))
        rm1, rv1 = bn.running_mean.double().cpu(), bn.running_var.double().cpu()   # after the recorded call's update
        ops.pn_pool_tap = []
        out = ops.pn_pool(ag, B, N, conv, bn, relu, training)
        tap = ops.pn_pool_tap[0]
    finally:
        ops.pn_pool_tap = None
    assert any(t.startswith("pn_pool_scan_kernel") for t in tags), tags
    (out * up.cuda()).sum().backward()
    P = {n: p.detach().cpu().double().requires_grad_(True) for n, p in
         (("w", conv.weight.view(C, K)), ("b", conv.bias), ("g", bn.weight), ("be", bn.bias))}
    ad = a0.double().requires_grad_(True)
    route = tap["route"].cpu()
    assert int(route.min()) >= 0 and int(route.max()) < N
    ref, mu, var = _pool_ref(ad, P["w"], P["b"], P["g"], P["be"], route, B, N, relu, training, rm0.double(), rv0.double())
    (ref * up.double()).sum().backward()
    # the routes are the argmax of the float64 evaluation (up to near-ties)
    zd = (ad @ P["w"].t() + P["b"]).detach().view(B, N, C)
    sel = zd.gather(1, route.long().unsqueeze(1)).squeeze(1)
    ext = torch.where(P["g"].detach() >= 0, zd.max(1).values, zd.min(1).values)
    assert float((sel - ext).abs().max()) < 1e-4
    assert relmax(out, ref) < 1e-5
    assert relmax(ag.grad, ad.grad) < 1e-5
    assert relmax(conv.weight.grad.view(C, K), P["w"].grad) < 1e-5
    assert relmax(bn.weight.grad, P["g"].grad) < 1e-5
    assert relmax(bn.bias.grad, P["be"].grad) < 1e-5
    if training:
        assert float(conv.bias.grad.abs().max()) == 0.0
        M = B * N
        assert relmax(bn.running_mean, 0.9 * rm1 + 0.1 * mu.detach()) < 1e-6
        assert relmax(bn.running_var, 0.9 * rv1 + 0.1 * var.detach() * M / (M - 1)) < 1e-6
    else:
        assert relmax(conv.bias.grad, P["b"].grad) < 1e-5
        assert torch.equal(bn.running_mean.cpu(), rm0)


# ------------------------------------------------------------------------------------------------ float64 restatement
def _bn(P, pre, z, training):
    if training:
        mu, var = z.mean(0), z.var(0, unbiased=False)
        if "_stats" in P:
            P["_stats"][pre] = (mu.detach(), var.detach(), z.shape[0])
    else:
        mu, var = P[pre + ".running_mean"], P[pre + ".running_var"]
    return (z - mu) / torch.sqrt(var + 1e-5) * P[pre + ".weight"] + P[pre + ".bias"]


def _conv(P, pre, h):
    w = P[pre + ".weight"]
    return h @ w.view(w.shape[0], -1).t() + P[pre + ".bias"]


def _lin(P, pre, h):
    return h @ P[pre + ".weight"].t() + P[pre + ".bias"]


def _act(P, v):
    """ReLU; with P["_relu"] (an iterator over the HIP path's ReLU decisions, in call order) the decisions are injected."""
    it = P.get("_relu")
    return torch.relu(v) if it is None else v * next(it).to(v)


def _gather(z, B, N, route):
    return z.view(B, N, -1).gather(1, route.long().unsqueeze(1)).squeeze(1)


def _tnet(P, pre, rows, B, N, k, route, tr):
    h = _act(P, _bn(P, pre + ".bn1", _conv(P, pre + ".conv1", rows), tr))
    h = _act(P, _bn(P, pre + ".bn2", _conv(P, pre + ".conv2", h), tr))
    g = _gather(torch.relu(_bn(P, pre + ".bn3", _conv(P, pre + ".conv3", h), tr)), B, N, route)
    g = _act(P, _bn(P, pre + ".bn4", _lin(P, pre + ".fc1", g), tr))
    g = _act(P, _bn(P, pre + ".bn5", _lin(P, pre + ".fc2", g), tr))
    return (_lin(P, pre + ".fc3", g) + torch.eye(k, dtype=g.dtype, device=g.device).flatten()).view(B, k, k)


def encoder_ref(P, pre, x, routes, tr, feature_transform, global_feat):
    """x (B, N, D) float64 -> the reference's PointNetEncoder outputs, max-pools taken at `routes` (the HIP path's, in call order)."""
    B, N, D = x.shape
    it = iter(routes)
    trans = _tnet(P, pre + ".stn", x.reshape(B * N, D), B, N, 3, next(it), tr)
    y = torch.cat([torch.bmm(x[..., :3], trans), x[..., 3:]], 2).reshape(B * N, D)
    h = _act(P, _bn(P, pre + ".bn1", _conv(P, pre + ".conv1", y), tr))
    tf = None
    if feature_transform:
        tf = _tnet(P, pre + ".fstn", h, B, N, 64, next(it), tr)
        h = torch.bmm(h.view(B, N, 64), tf).reshape(B * N, 64)
    pf = h
    h = _act(P, _bn(P, pre + ".bn2", _conv(P, pre + ".conv2", h), tr))
    g = _gather(_bn(P, pre + ".bn3", _conv(P, pre + ".conv3", h), tr), B, N, next(it))
    if global_feat:
        return g, trans, tf
    return torch.cat([g.unsqueeze(2).expand(B, 1024, N), pf.view(B, N, 64).transpose(1, 2)], 1), trans, tf


def pointnet_ref(P, x, routes, mask, tr, feature_transform):
    g, trans, tf = encoder_ref(P, "encoder", x, routes, tr, feature_transform, True)
    h = _act(P, _bn(P, "bn1", _lin(P, "fc1", g), tr))
    h = _lin(P, "fc2", h)
    if tr:
        h = h * mask / 0.6
    h = _act(P, _bn(P, "bn2", h, tr))
    return _lin(P, "fc3", h), trans, tf


def _params64(state, device="cpu"):
    return {k: (v.detach().to(device).double().requires_grad_(True) if v.is_floating_point() else v.to(device))
            for k, v in state.items()}


class _ReluDecisions:
    """Records the ReLU decisions of the per-point layers and the heads (ops.fc_block with relu, the narrow layers of ops.pn_trunk,
    ops.pn_bn_relu) in call order."""

    def __enter__(self):
        from pnpp_hip import ops
        self.masks, self.fc, self.bn = [], ops.fc_block, ops.pn_bn_relu

        def fc(*a, **k):
            y = self.fc(*a, **k)
            if k.get("relu", False):
                self.masks.append((y.detach() > 0).cpu())
            return y

        def bn(*a, **k):
            y = self.bn(*a, **k)
            self.masks.append((y.detach() > 0).cpu())
            return y

        ops.fc_block, ops.pn_bn_relu = fc, bn
        ops.pn_relu_tap = self.masks          # the narrow layers inside ops.pn_trunk
        return self

    def __exit__(self, *exc):
        from pnpp_hip import ops
        ops.fc_block, ops.pn_bn_relu = self.fc, self.bn
        ops.pn_relu_tap = None


def _run_model(model, x, mask, t, relu_out=None):
    from pnpp_hip import ops
    ops.pn_pool_tap = []
    try:
        with _ReluDecisions() as rd:
            out, trans, trans_feat = model(x, drop_mask=mask, return_transforms=True)
        routes = [d["route"].clone() for d in ops.pn_pool_tap]
        if relu_out is not None:
            relu_out.extend(rd.masks)
    finally:
        ops.pn_pool_tap = None
    loss = ops.mse_rows(out, t).mean()
    if trans_feat is not None:
        loss = loss + 0.001 * ops.feature_transform_regularizer(trans_feat)
    return out, loss, routes, trans, trans_feat


def _reg64(tf):
    k = tf.shape[1]
    return (torch.bmm(tf, tf.transpose(1, 2)) - torch.eye(k, dtype=tf.dtype, device=tf.device)).flatten(1).norm(dim=1).mean()


def _check_model(B, N, feature_transform, dev64, gate_vals, gate_grad):
    from models.pointnet import PointNet
    torch.manual_seed(11)
    m = PointNet(feature_transform)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda().train()
    g = torch.Generator().manual_seed(B + N)
    x = torch.randn(B, N, 3, generator=g)
    t = torch.randn(B, 3, generator=g)
    mask = (torch.rand(B, 256, generator=g) < 0.6).to(torch.uint8)
    relu = []
    out, loss, routes, trans, trans_feat = _run_model(m, x.cuda(), mask.cuda(), t.cuda(), relu)
    loss.backward()
    P = _params64(state, dev64)
    P["_relu"] = iter(relu)
    o64, tr64, tf64 = pointnet_ref(P, x.double().to(dev64), [r.to(dev64) for r in routes], mask.double().to(dev64), True,
                                   feature_transform)
    l64 = ((o64 - t.double().to(dev64)) ** 2).mean()
    if feature_transform:
        l64 = l64 + 0.001 * _reg64(tf64)
    l64.backward()
    assert len(routes) == (3 if feature_transform else 2)
    assert relmax(out, o64) < gate_vals
    assert relmax(trans, tr64) < gate_vals
    if feature_transform:
        assert relmax(trans_feat, tf64) < gate_vals
    else:
        assert trans_feat is None
    assert abs(float(loss) - float(l64)) <= gate_vals * abs(float(l64))
    names = [n for n, _ in m.named_parameters()]
    got = torch.cat([dict(m.named_parameters())[n].grad.detach().double().cpu().flatten() for n in names])
    ref = torch.cat([P[n].grad.detach().cpu().flatten() for n in names])
    err = float((got - ref).norm() / ref.norm())
    assert err < gate_grad, err
    # running statistics after the step
    for n, b in m.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            assert torch.isfinite(b).all(), n
    return m, state, err


@pytest.mark.parametrize("feature_transform", [True, False])
def test_pointnet_vs_float64(feature_transform):
    _check_model(16, 256, feature_transform, "cpu", 1e-4, 1e-4)


def test_encoder_channel6_pointwise_vs_float64():
    """PointNetEncoder(global_feat=False, feature_transform=True, channel=6): (B, 1088, N) output, extra columns passed through
    the input transform, and the backward pass of the broadcast-concat."""
    from models.pointnet import PointNetEncoder
    from pnpp_hip import ops
    B, N = 4, 200
    torch.manual_seed(3)
    enc = PointNetEncoder(global_feat=False, feature_transform=True, channel=6)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    enc = enc.cuda().train()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, 6, N, generator=g)
    up = torch.randn(B, 1088, N, generator=g)
    ops.pn_pool_tap = []
    try:
        with _ReluDecisions() as rd:
            out, trans, tf = enc(x.cuda())
        routes = [d["route"].cpu() for d in ops.pn_pool_tap]
    finally:
        ops.pn_pool_tap = None
    assert out.shape == (B, 1088, N) and trans.shape == (B, 3, 3) and tf.shape == (B, 64, 64)
    ((out * up.cuda()).sum() + ops.feature_transform_regularizer(tf)).backward()
    P = {"enc." + k: v for k, v in _params64(state).items()}
    P["_relu"] = iter(rd.masks)
    o64, tr64, tf64 = encoder_ref(P, "enc", x.double().transpose(1, 2), routes, True, True, False)
    ((o64 * up.double()).sum() + _reg64(tf64)).backward()
    assert relmax(out, o64) < 1e-4 and relmax(trans, tr64) < 1e-4 and relmax(tf, tf64) < 1e-4
    names = [n for n, _ in enc.named_parameters()]
    got = torch.cat([dict(enc.named_parameters())[n].grad.double().cpu().flatten() for n in names])
    ref = torch.cat([P["enc." + n].grad.flatten() for n in names])
    assert float((got - ref).norm() / ref.norm()) < 1e-4


def test_pointnet_eval_mode_vs_float64():
    from models.pointnet import PointNet
    B, N = 8, 640                                           # 5120 rows: the per-point BatchNorm backward of many rows, eval form
    torch.manual_seed(2)
    m = PointNet(True).cuda().train()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        m(torch.randn(B, N, 3, generator=g).cuda())        # one train-mode pass: running statistics move off their init
    m.eval()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.randn(B, N, 3, generator=g)
    t = torch.randn(B, 3, generator=g)
    relu = []
    out, loss, routes = _run_model(m, x.cuda(), None, t.cuda(), relu)[:3]
    loss.backward()
    P = _params64(state)
    P["_relu"] = iter(relu)
    o64, _, tf64 = pointnet_ref(P, x.double(), [r.cpu() for r in routes], None, False, True)
    (((o64 - t.double()) ** 2).mean() + 0.001 * _reg64(tf64)).backward()
    assert relmax(out, o64) < 1e-4
    names = [n for n, _ in m.named_parameters()]
    got = torch.cat([dict(m.named_parameters())[n].grad.double().cpu().flatten() for n in names])
    ref = torch.cat([P[n].grad.flatten() for n in names])
    assert float((got - ref).norm() / ref.norm()) < 1e-4


def test_pointnet_full_size_routed_and_saved_bytes():
    """B = 32, N = 1024: against the float64 restatement (evaluated on the GPU) with the max routes injected; the bytes kept for
    backward hold none of the (B*N) x 1024 activations."""
    from models.pointnet import PointNet
    from pnpp_hip import ops
    B, N = 32, 1024
    torch.manual_seed(11)
    m = PointNet(True)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda().train()
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(B, N, 3, generator=g).cuda(), torch.randn(B, 3, generator=g).cuda()
    mask = (torch.rand(B, 256, generator=g) < 0.6).to(torch.uint8).cuda()
    seen, total = set(), [0]

    def pack(tensor):
        key = (tensor.untyped_storage().data_ptr(), tensor.untyped_storage().nbytes())
        if tensor.is_cuda and key not in seen and not isinstance(tensor, torch.nn.Parameter):
            seen.add(key)
            total[0] += key[1]
        return tensor

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t_: t_):
        relu = []
        out, loss, routes, trans, tf = _run_model(m, x, mask, t, relu)
    assert total[0] < B * N * 1024 * 4, total[0]
    loss.backward()
    P = _params64(state, "cuda")
    P["_relu"], P["_stats"] = iter(relu), {}
    o64, tr64, tf64 = pointnet_ref(P, x.double(), routes, mask.double(), True, True)
    l64 = ((o64 - t.double()) ** 2).mean() + 0.001 * _reg64(tf64)
    l64.backward()
    assert relmax(out, o64) < 1e-5
    assert relmax(trans, tr64) < 1e-5 and relmax(tf, tf64) < 1e-5
    bufs = dict(m.named_buffers())
    for pre, (mu, var, M) in P["_stats"].items():
        assert relmax(bufs[pre + ".running_mean"], 0.9 * state[pre + ".running_mean"].double().cuda() + 0.1 * mu) < 1e-5, pre
        assert relmax(bufs[pre + ".running_var"], 0.9 * state[pre + ".running_var"].double().cuda() + 0.1 * var * M / (M - 1)) < 1e-5, pre
    names = [n for n, _ in m.named_parameters()]
    got = torch.cat([dict(m.named_parameters())[n].grad.double().flatten() for n in names])
    ref = torch.cat([P[n].grad.flatten() for n in names])
    err = float((got - ref).norm() / ref.norm())
    print(f"full size: flat gradient rel err {err:.2e}, saved {total[0] / 2**20:.1f} MiB")
    assert err < ROUTED_GATE, err


# ------------------------------------------------------------------------------------------------ determinism, capture, training
def test_two_identical_steps_bitwise():
    from models.pointnet import PointNet
    torch.manual_seed(5)
    m1 = PointNet(True).cuda().train()
    m2 = copy.deepcopy(m1)
    g = torch.Generator().manual_seed(2)
    x, t = torch.randn(16, 512, 3, generator=g).cuda(), torch.randn(16, 3, generator=g).cuda()
    mask = (torch.rand(16, 256, generator=g) < 0.6).to(torch.uint8).cuda()
    for m in (m1, m2):
        _run_model(m, x, mask, t)[1].backward()
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_hipgraph_step_with_captured_adam_equals_eager():
    from models.pointnet import PointNet
    from pnpp_hip import ops, optim
    from pnpp_hip.graph import GraphedStep
    torch.manual_seed(7)
    m1 = PointNet(True).cuda().train()
    m1.dropout.p = 0.0                                    # dropout draws differ between capture and eager streams
    m2 = copy.deepcopy(m1)
    o1, o2 = optim.FlatAdam(m1.parameters(), lr=1e-3), optim.FlatAdam(m2.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(3)
    x, t = torch.randn(8, 256, 3, generator=g).cuda(), torch.randn(8, 3, generator=g).cuda()

    def loss_fn(model):
        def f(xx, tt):
            out, _, tf = model(xx, return_transforms=True)
            return ops.mse_rows(out, tt).mean() + 0.001 * ops.feature_transform_regularizer(tf)
        return f

    gs = GraphedStep(o1, loss_fn(m1), [x, t], fused_optimizer=True)
    assert torch.equal(o1.flat_p, o2.flat_p)
    for p, q in zip(m1.buffers(), m2.buffers()):
        p.copy_(q)
    for it in range(3):
        l1 = float(gs(x, t))
        o2.zero_grad()
        l2 = loss_fn(m2)(x, t)
        l2.backward()
        o2.step()
        assert l1 == float(l2), (it, l1, float(l2))
        assert torch.equal(o1.flat_p, o2.flat_p), it
    assert torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)


def test_training_loss_decreases():
    import synthetic
    from models.pointnet import PointNet
    from pnpp_hip import ops, optim
    torch.manual_seed(0)
    m = PointNet(True).cuda().train()
    opt = optim.FlatAdam(m.parameters(), lr=1e-3)
    xyz, _, _, fwd = synthetic.rotated_clouds(16, 512, seed=5)
    xyz, fwd = xyz.cuda(), fwd.cuda()
    losses = []
    for _ in range(50):
        opt.zero_grad()
        out, _, tf = m(xyz, return_transforms=True)
        loss = ops.mse_rows(out, fwd).mean() + 0.001 * ops.feature_transform_regularizer(tf)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(map(lambda v: v == v, losses))
    assert sum(losses[-5:]) / 5 < 0.5 * sum(losses[:5]) / 5, losses


# ------------------------------------------------------------------------------------------------ against the reference's capture
def _check_grads(g, tag, model):
    import math
    import numpy as np
    worst = 0.0
    # the loss's gradient scale: the encoder case's sum(out * up) has gradients of ~1e6, the PointNet cases of ~10
    scale = max(float(g[k]) for k in g.files if k.startswith(f"{tag}.gn."))
    for n, p in model.named_parameters():
        pos, ref, norm = g[f"{tag}.gp.{n}"], g[f"{tag}.gs.{n}"], float(g[f"{tag}.gn.{n}"])
        if norm < max(1e-5, 1e-10 * scale):   # biases in front of a train-mode BatchNorm: zero in exact arithmetic
            assert float(p.grad.abs().max()) <= max(1e-5, 1e-8 * scale), n
            continue
        got = p.grad.detach().cpu().double().flatten()[torch.from_numpy(pos)].numpy()
        worst = max(worst, float(np.abs(got - ref).max() / (norm / math.sqrt(p.numel()))))
        gn = float(p.grad.detach().double().norm())
        assert abs(gn - norm) <= 1e-3 * norm, (tag, n, gn, norm)
    assert worst <= 2e-2, (tag, worst)
    return worst


def _check_after(g, tag, model, prefix=""):
    import numpy as np
    for k, v in model.state_dict().items():
        if "running" in k:
            assert np.allclose(v.cpu().double().numpy(), g[f"{tag}.after.{prefix}{k}"], rtol=1e-4, atol=1e-6), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k


@pytest.mark.parametrize("tag", ["ft", "noft"])
def test_pointnet_vs_reference_capture(golden, tag):
    """16 clouds of 256 points against the reference's own module in float64 (tests/golden/pointnet.npz): outputs, trans,
    trans_feat, loss, gradients, running statistics after the step and the eval-mode outputs after it."""
    import numpy as np
    from models.pointnet import PointNet
    from pnpp_hip import ops
    g = golden("pointnet.npz")
    torch.manual_seed(int(g[f"{tag}.seed"]))
    m = PointNet(tag == "ft").cuda().train()
    x, t, mask = (torch.from_numpy(g[f"{tag}.{k}"]).cuda() for k in ("x", "t", "mask"))
    out, trans, tf = m(x, drop_mask=mask, return_transforms=True)
    loss = ops.mse_rows(out, t).mean()
    if tf is not None:
        loss = loss + 0.001 * ops.feature_transform_regularizer(tf)
    loss.backward()
    assert np.abs(out.detach().cpu().double().numpy() - g[f"{tag}.out"]).max() < 2e-5
    assert np.abs(trans.detach().cpu().double().numpy() - g[f"{tag}.trans"]).max() < 2e-5
    if tag == "ft":
        assert np.abs(tf.detach().cpu().double().numpy() - g[f"{tag}.trans_feat"]).max() < 2e-5
    else:
        assert tf is None
    assert abs(float(loss.detach()) - float(g[f"{tag}.loss"])) <= 1e-5 * max(1.0, abs(float(g[f"{tag}.loss"])))
    worst = _check_grads(g, tag, m)
    _check_after(g, tag, m)
    m.eval()
    with torch.no_grad():
        ev = m(x)
    assert np.abs(ev.cpu().double().numpy() - g[f"{tag}.eval_out"]).max() < 5e-5
    print(f"\n[pointnet {tag}] loss {float(loss):.7f} ref {float(g[f'{tag}.loss']):.7f} worst sampled grad err {worst:.2e}")


def test_encoder_channel6_vs_reference_capture(golden):
    import numpy as np
    from models.pointnet import PointNetEncoder
    from pnpp_hip import ops
    g = golden("pointnet.npz")
    seed = int(g["enc6.seed"])
    torch.manual_seed(seed)
    enc = PointNetEncoder(global_feat=False, feature_transform=True, channel=6).cuda().train()
    gen = torch.Generator().manual_seed(1000 + seed)
    torch.randn(16, 6, 256, generator=gen, dtype=torch.float64)           # x (stored), then the upstream gradient
    up = torch.randn(16, 1088, 256, generator=gen, dtype=torch.float64).float().cuda()
    x = torch.from_numpy(g["enc6.x"]).cuda()
    out, trans, tf = enc(x)
    (out * up).sum().backward()
    pos = torch.from_numpy(g["enc6.out_pos"])
    norm = float(g["enc6.out_n"])
    assert np.abs(out.detach().flatten().cpu()[pos].double().numpy() - g["enc6.out_s"]).max() < 2e-5 * max(1.0, norm / 1e3)
    assert abs(float(out.detach().double().norm()) - norm) <= 1e-5 * norm
    assert np.abs(trans.detach().cpu().double().numpy() - g["enc6.trans"]).max() < 2e-5
    assert np.abs(tf.detach().cpu().double().numpy() - g["enc6.trans_feat"]).max() < 2e-5
    _check_grads(g, "enc6", enc)
    _check_after(g, "enc6", enc)
    enc.eval()
    with torch.no_grad():
        ev = enc(x)[0].flatten().cpu()
    assert np.abs(ev[pos].double().numpy() - g["enc6.eval_s"]).max() < 5e-5 * max(1.0, norm / 1e3)
