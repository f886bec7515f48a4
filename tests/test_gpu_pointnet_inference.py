"""Forward-only path of the vanilla PointNet models (pnpp_hip.pointnet_inference, csrc/pointnet_infer_kernels.hip) against a float64
eval-mode evaluation and against the library's existing eval path.  Gates, the project's own (tests/test_gpu_inference.py): folded
parameters <= 1 ulp of the float64 formula rounded to float32; a trunk's pooled output, trans, trans_feat and the global feature
<= 1e-5 of the tensor's max-abs (G2); whole-model outputs <= 1e-4 * max(1, max|ref|).

The float64 side is the restatement of tests/test_gpu_pointnet.py (_conv, _bn, _lin in eval mode) with a true max over the points:
the forward value is continuous in its inputs, so no route or ReLU decision of the HIP path is injected."""
import math

import numpy as np
import pytest
import torch

import test_gpu_pointnet as tp
from conftest import has_gpu, relmax

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an AMD GPU")]

G2 = 1e-5


# ------------------------------------------------------------------------------------------------ float64 eval-mode restatement
def _layer64(P, pre, i, h, relu=True):
    z = tp._bn(P, f"{pre}.bn{i}", tp._conv(P, f"{pre}.conv{i}", h), False)
    return torch.relu(z) if relu else z


def _tnet_pooled64(P, pre, rows, B, N):
    h = _layer64(P, pre, 2, _layer64(P, pre, 1, rows))
    return _layer64(P, pre, 3, h).view(B, N, -1).max(1).values


def _tnet_head64(P, pre, g, k):
    g = torch.relu(tp._bn(P, pre + ".bn4", tp._lin(P, pre + ".fc1", g), False))
    g = torch.relu(tp._bn(P, pre + ".bn5", tp._lin(P, pre + ".fc2", g), False))
    return (tp._lin(P, pre + ".fc3", g) + torch.eye(k, dtype=g.dtype).flatten()).view(-1, k, k)


def _enc_h64(P, pre, x, trans):
    B, N, D = x.shape
    y = torch.cat([torch.bmm(x[..., :3], trans), x[..., 3:]], 2).reshape(B * N, D)
    return _layer64(P, pre, 1, y)


def _enc_pooled64(P, pre, h, B, N, trans_feat):
    if trans_feat is not None:
        h = torch.bmm(h.view(B, N, 64), trans_feat).reshape(B * N, 64)
    g = _layer64(P, pre, 3, _layer64(P, pre, 2, h), relu=False).view(B, N, -1).max(1).values
    return g, h


def encoder64(P, pre, x, feature_transform, global_feat=True):
    """x (B, N, D) float64 -> (output, trans, trans_feat, global feature) of the reference's PointNetEncoder in eval mode"""
    B, N, D = x.shape
    trans = _tnet_head64(P, pre + ".stn", _tnet_pooled64(P, pre + ".stn", x.reshape(B * N, D), B, N), 3)
    h = _enc_h64(P, pre, x, trans)
    tf = _tnet_head64(P, pre + ".fstn", _tnet_pooled64(P, pre + ".fstn", h, B, N), 64) if feature_transform else None
    g, pf = _enc_pooled64(P, pre, h, B, N, tf)
    out = g if global_feat else torch.cat([g.unsqueeze(2).expand(B, 1024, N), pf.view(B, N, 64).transpose(1, 2)], 1)
    return out, trans, tf, g


def pointnet64(P, x, feature_transform):
    g, trans, tf, _ = encoder64(P, "encoder", x, feature_transform)
    h = torch.relu(tp._bn(P, "bn1", tp._lin(P, "fc1", g), False))
    h = torch.relu(tp._bn(P, "bn2", tp._lin(P, "fc2", h), False))   # dropout is the identity in eval mode
    return tp._lin(P, "fc3", h), trans, tf, g


# ------------------------------------------------------------------------------------------------ models and inputs
def _randomise(model, seed, negative_gamma=True):
    """BatchNorm affine parameters and running statistics off their initial values (tests/test_gpu_inference.py::_randomise:
    running_var log-uniform in [0.05, 2]); a share of the encoder's bn3 gets gamma < 0 (its folded W' carries the sign)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                n = m.num_features
                m.weight.copy_(0.5 + torch.rand(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(n, generator=g))
                m.running_var.copy_(torch.exp(math.log(0.05) + torch.rand(n, generator=g) * (math.log(2.0) - math.log(0.05))))
        if negative_gamma:
            enc = getattr(model, "encoder", model)
            enc.bn3.weight[::7].mul_(-1.0)
            assert int((enc.bn3.weight < 0).sum()) >= 50
    return model


def _state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _p64(state, prefix=""):
    return {prefix + k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}


def _pointnet(feature_transform, seed=3):
    from models.pointnet import PointNet
    torch.manual_seed(seed)
    m = _randomise(PointNet(feature_transform), seed + 100)
    return m.cuda().eval(), _state(m)


def _encoder(seed=3, **kw):
    from models.pointnet import PointNetEncoder
    torch.manual_seed(seed)
    m = _randomise(PointNetEncoder(**kw), seed + 100)
    return m.cuda().eval(), _state(m)


def _cloud(B, N, D, seed):
    """(B, N, D) points with exact ties: every cloud repeats some of its own points"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, D, generator=g)
    if N >= 4:
        x[:, N // 2] = x[:, 0]
        x[:, N - 1] = x[:, 1]
    return x


def _gate_eval(got, ref, what):
    ref = ref.detach().double()
    d = float((got.detach().cpu().double().reshape(ref.shape) - ref).abs().max())
    gate = 1e-4 * max(1.0, float(ref.abs().max()))
    print(f"  {what}: |predictor - float64| = {d:.3e} (gate {gate:.1e})")
    assert d <= gate, what


def _g2(got, ref, what, extra=""):
    e = relmax(got, ref)
    print(f"  {what}: relmax {e:.3e} (gate {G2:.0e}){extra}")
    assert e <= G2, what


# ------------------------------------------------------------------------------------------------ fold
def test_fold_matches_float64_formula():
    from pnpp_hip.inference import Predictor
    model, state = _pointnet(True)
    p = Predictor(model)
    torch.cuda.synchronize()
    assert p.plan == {k: "fused" for k in ("stn", "stn.fc1", "stn.fc2", "fstn", "fstn.fc1", "fstn.fc2", "encoder", "fc1", "fc2")}

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

    chains = {"stn": [("encoder.stn.conv%d" % i, "encoder.stn.bn%d" % i) for i in (1, 2, 3)],
              "fstn": [("encoder.conv1", "encoder.bn1")] + [("encoder.fstn.conv%d" % i, "encoder.fstn.bn%d" % i) for i in (1, 2, 3)],
              "encoder": [("encoder.conv%d" % i, "encoder.bn%d" % i) for i in (1, 2, 3)]}
    for trunk, chain in chains.items():
        for l, (conv, bn) in enumerate(chain):
            w, b, pad = p.folded_layer(trunk, l)
            wr, br = formula(state[conv + ".weight"], state[conv + ".bias"], bn)
            uw, ub = ulps(w, wr), ulps(b, br)
            print(f"  {trunk} layer {l}: W' {uw:.2f} ulp, b' {ub:.2f} ulp")
            assert uw <= 1.0 and ub <= 1.0, (trunk, l)
            assert pad.numel() == 0 or float(pad.abs().max()) == 0.0
    heads = {"stn.fc1": ("encoder.stn.fc1", "encoder.stn.bn4"), "stn.fc2": ("encoder.stn.fc2", "encoder.stn.bn5"),
             "fstn.fc1": ("encoder.fstn.fc1", "encoder.fstn.bn4"), "fstn.fc2": ("encoder.fstn.fc2", "encoder.fstn.bn5"),
             "fc1": ("fc1", "bn1"), "fc2": ("fc2", "bn2")}
    for name, (fc, bn) in heads.items():
        f = p._heads[name]
        wr, br = formula(state[fc + ".weight"], state[fc + ".bias"], bn)
        assert ulps(f.weight, wr) <= 1.0 and ulps(f.bias, br) <= 1.0, name


# ------------------------------------------------------------------------------------------------ each trunk kernel alone
SIZES = [(32, 1024), (1, 1024), (36, 777), (3, 2500), (2, 10000), (5, 1), (4, 33)]


@pytest.mark.parametrize("feature_transform,D", [(True, 3), (True, 6), (False, 3)], ids=["ft-D3", "ft-D6", "noft-D3"])
@pytest.mark.parametrize("B,N", SIZES, ids=[f"{b}x{n}" for b, n in SIZES])
def test_trunk_parity_g2(B, N, D, feature_transform):
    """Every trunk launch on its own: all paths get the float64 evaluation's transforms (rounded to float32) as their inputs."""
    from pnpp_hip.inference import Predictor
    enc, state = _encoder(global_feat=True, feature_transform=feature_transform, channel=D)
    assert int((enc.bn3.weight < 0).sum()) >= 50
    P = _p64(state, "e.")
    p = Predictor(enc)
    x = _cloud(B, N, D, seed=B * 100003 + N)
    x64 = x.double()
    with torch.no_grad():
        trans = _tnet_head64(P, "e.stn", _tnet_pooled64(P, "e.stn", x64.reshape(B * N, D), B, N), 3).float()
        h = _enc_h64(P, "e", x64, trans.double())
        refs = {"stn": _tnet_pooled64(P, "e.stn", x64.reshape(B * N, D), B, N)}
        tf = None
        if feature_transform:
            refs["fstn"] = _tnet_pooled64(P, "e.fstn", h, B, N)
            tf = _tnet_head64(P, "e.fstn", refs["fstn"], 64).float()
        refs["encoder"] = _enc_pooled64(P, "e", h, B, N, None if tf is None else tf.double())[0]
        layouts = {"bdn": x.transpose(1, 2).contiguous().cuda().transpose(1, 2),   # (B, D, N) storage read through strides
                   "bnd": x.cuda()}
        tg, tfg = trans.cuda(), None if tf is None else tf.cuda()
        for name, ref in refs.items():
            outs = {}
            for lay, xr in layouts.items():
                out, _ = p._trunk(name, xr, None if name == "stn" else tg, tfg if name == "encoder" else None)
                assert p.last_plan[name] == "fused" and out.shape == ref.shape and not out.requires_grad
                outs[lay] = out.clone()
            torch.cuda.synchronize()
            assert torch.equal(outs["bdn"], outs["bnd"]), f"{name}: the two input layouts differ"
            extra = ""
            if B * N > 32:
                ev, _ = p._eval_trunk(name, layouts["bnd"], None if name == "stn" else tg, tfg if name == "encoder" else None)
                extra = f"   existing eval path {relmax(ev, ref):.3e}"
            _g2(outs["bnd"], ref, f"{name} B={B} N={N} D={D}", extra)


# ------------------------------------------------------------------------------------------------ whole models
def _check_pointnet(feature_transform, B, N, layout):
    from pnpp_hip.inference import Predictor
    model, state = _pointnet(feature_transform)
    p = Predictor(model)
    x = _cloud(B, N, 3, seed=77 + N)
    xg = x.cuda() if layout == "bnd" else x.transpose(1, 2).contiguous().cuda()
    with torch.no_grad():
        got = p(xg, return_transforms=True)
        ev = model(xg, return_transforms=True)
        ref = pointnet64(_p64(state), x.double(), feature_transform)
    torch.cuda.synchronize()
    assert p.last_plan == p.plan and set(p.plan.values()) == {"fused"}
    assert isinstance(got, tuple) and len(got) == 3
    for g, e in zip(got, ev):
        assert (g is None) == (e is None)
        if g is not None:
            assert g.shape == e.shape and g.dtype == e.dtype and g.device == e.device and not g.requires_grad
    _gate_eval(got[0], ref[0], f"PointNet({feature_transform}) {B}x{N} out")
    print(f"  |predictor - model.eval()| = {float((got[0] - ev[0]).abs().max()):.3e}; model.eval() vs float64 {relmax(ev[0], ref[0]):.3e}")
    _g2(got[1], ref[1], "trans")
    if feature_transform:
        _g2(got[2], ref[2], "trans_feat")
    single = p(xg)
    assert torch.is_tensor(single) and torch.equal(single, got[0])
    return p


@pytest.mark.parametrize("feature_transform", [True, False])
@pytest.mark.parametrize("B,N,layout", [(32, 1024, "bnd"), (3, 2500, "bdn"), (2, 17, "bnd"), (1, 1, "bdn")])
def test_whole_pointnet(feature_transform, B, N, layout):
    if B * N <= 32:   # model.eval() itself refuses these sizes (ops.pn_trunk); the Predictor runs them
        from pnpp_hip.inference import Predictor
        model, state = _pointnet(feature_transform)
        x = _cloud(B, N, 3, seed=5)
        xg = x.cuda() if layout == "bnd" else x.transpose(1, 2).contiguous().cuda()
        got = Predictor(model)(xg, return_transforms=True)
        ref = pointnet64(_p64(state), x.double(), feature_transform)
        _gate_eval(got[0], ref[0], f"PointNet({feature_transform}) {B}x{N} out")
        _g2(got[1], ref[1], "trans")
        return
    _check_pointnet(feature_transform, B, N, layout)


def test_whole_encoder_channel6_pointwise():
    from pnpp_hip.inference import Predictor
    B, N = 4, 777
    enc, state = _encoder(global_feat=False, feature_transform=True, channel=6)
    p = Predictor(enc)
    x = _cloud(B, N, 6, seed=9).transpose(1, 2).contiguous()   # (B, 6, N)
    with torch.no_grad():
        got = p(x.cuda())
        ev = enc(x.cuda())
        out64, tr64, tf64, g64 = encoder64(_p64(state, "e."), "e", x.double().transpose(1, 2), True, global_feat=False)
    assert got[0].shape == (B, 1088, N) == ev[0].shape and got[1].shape == (B, 3, 3) and got[2].shape == (B, 64, 64)
    _g2(got[0][:, :1024, 0], g64, "global feature")
    _g2(got[0][:, 1024:], out64[:, 1024:], "point features")
    _g2(got[1], tr64, "trans")
    _g2(got[2], tf64, "trans_feat")
    _gate_eval(got[0], out64, "encoder output")
    print(f"  |predictor - encoder.eval()| = {float((got[0] - ev[0]).abs().max()):.3e}")
    with pytest.raises(ValueError, match="expected input with 6 channels"):
        p(torch.zeros(B, 3, N, device="cuda"))
    with pytest.raises(ValueError, match="expected input with 6 channels"):
        enc(torch.zeros(B, 3, N, device="cuda"))
    # global_feat=True returns the pooled feature itself: not a buffer the next call overwrites
    enc2, _ = _encoder(global_feat=True, feature_transform=False, channel=3)
    p2 = Predictor(enc2)
    a = p2(torch.randn(2, 3, 100, device="cuda"))[0]
    keep = a.clone()
    p2(torch.randn(2, 3, 100, device="cuda"))
    assert torch.equal(a, keep) and p2(torch.randn(2, 3, 100, device="cuda"))[2] is None


def _load_bn(model, bits):
    vals = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).float()
    at = 0
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                for t in (m.weight, m.bias, m.running_mean, m.running_var):
                    t.copy_(vals[at:at + t.numel()])
                    at += t.numel()
    return at


@pytest.mark.parametrize("tag", ["ft", "noft", "enc6"])
def test_against_the_reference_modules_fixture(golden, tag):
    """tests/golden/pointnet_infer.npz: the reference's own module in float64 eval mode (tools/make_golden_pointnet_infer.py)"""
    from pnpp_hip.inference import Predictor
    from models.pointnet import PointNet, PointNetEncoder
    z = golden("pointnet_infer.npz")
    torch.manual_seed(int(z[f"{tag}.seed"]))
    model = PointNetEncoder(False, True, 6) if tag == "enc6" else PointNet(tag == "ft")
    bits = z["ft.bn" if tag == "enc6" else f"{tag}.bn"]
    used = _load_bn(model, bits)
    assert used == bits.size or tag == "enc6"
    p = Predictor(model.cuda().eval())
    x = torch.from_numpy(z[f"{tag}.x"]).cuda()
    if tag == "enc6":
        out, trans, tf = p(x)
        pos = torch.from_numpy(z["enc6.out_pos"].astype(np.int64))
        d = float((out.flatten().cpu().double()[pos] - torch.from_numpy(z["enc6.out_s"])).abs().max())
        gate = 1e-4 * max(1.0, float(z["enc6.out_absmax"]))
        print(f"  enc6 output samples: {d:.3e} (gate {gate:.1e})")
        assert d <= gate
        tpos = torch.from_numpy(z["enc6.tf_pos"].astype(np.int64))
        dt = float((tf.flatten().cpu().double()[tpos] - torch.from_numpy(z["enc6.tf_s"])).abs().max()) / float(z["enc6.tf_absmax"])
        print(f"  enc6 trans_feat samples: {dt:.3e} of max-abs")
        assert dt <= G2
        _g2(out[:, :1024, 0], torch.from_numpy(z["enc6.global"]), "enc6 global feature")
    else:
        out, trans, tf = p(x, return_transforms=True)
        _gate_eval(out, torch.from_numpy(z[f"{tag}.out"]), f"{tag} out")
        if tag == "ft":
            _g2(tf, torch.from_numpy(z["ft.trans_feat"]), "ft trans_feat")
        else:
            assert tf is None
        with torch.no_grad():   # the global feature: the encoder trunk on the transforms the Predictor just computed
            g, _ = p._trunk("encoder", x, trans, tf)
        _g2(g, torch.from_numpy(z[f"{tag}.global"]), f"{tag} global feature")
    _g2(trans, torch.from_numpy(z[f"{tag}.trans"]), f"{tag} trans")


# ------------------------------------------------------------------------------------------------ dispatch
@pytest.mark.parametrize("feature_transform", [True, False])
def test_dispatch_of_a_fused_forward(feature_transform):
    import dispatch
    from pnpp_hip.inference import Predictor
    B, N = 32, 1024
    model, _ = _pointnet(feature_transform)
    p = Predictor(model)
    x = _cloud(B, N, 3, seed=1).cuda()
    p(x)
    tags = dispatch.record(lambda: p(x))
    trunks = dispatch.find(tags, "pn_infer_kernel")
    assert len(trunks) == (3 if feature_transform else 2), tags   # one distinct tag per trunk
    assert len(dispatch.find(tags, "pn_infer_finish_kernel")) >= 1
    dispatch.expect(tags, absent=["pn_pool_scan_kernel", "pn_transform_kernel", "pn_gram_kernel"])
    assert not [t for t in tags if f"M={B * N}" in t.split()], tags       # no per-point layer ran as a launch of its own
    assert p.plan == p.last_plan and set(p.plan.values()) == {"fused"}
    ev_tags = dispatch.record(lambda: model(x))
    dispatch.expect(ev_tags, present=["pn_pool_scan_kernel"], absent=["pn_infer_kernel"])
    # small B: the pooled layer's columns are split over blockIdx.y
    x1 = _cloud(1, 1024, 3, seed=2).cuda()
    t1 = dispatch.record(lambda: p(x1))
    assert all(dispatch.field(t, "split") > 1 for t in dispatch.find(t1, "pn_infer_kernel")), t1
    assert all(dispatch.field(t, "split") == 1 for t in trunks), trunks


# ------------------------------------------------------------------------------------------------ refused shapes
def test_refused_width_takes_the_eval_path_bit_equal():
    """An encoder whose conv2 / bn2 / conv3 were replaced by modules with a width of 48: the kernel refuses the trunk (not a multiple
    of 32), the eval path takes it (pn_pool takes K = 4 .. 128)."""
    import torch.nn as nn
    from models.pointnet import _first_layer, _pad4
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    B, N = 4, 300
    model, _ = _pointnet(True)
    torch.manual_seed(1)
    enc = model.encoder
    enc.conv2, enc.bn2, enc.conv3 = nn.Conv1d(64, 48, 1).cuda(), nn.BatchNorm1d(48).cuda(), nn.Conv1d(48, 1024, 1).cuda()
    model.eval()
    p = Predictor(model)
    assert p.plan["encoder"] == "eval-path" and p.plan["stn"] == "fused" and p.plan["fstn"] == "fused"
    x = _cloud(B, N, 3, seed=3).cuda()
    with torch.no_grad():
        got = p(x, return_transforms=True)
        ref = model(x, return_transforms=True)
        assert p.last_plan["encoder"] == "eval-path" and p.last_plan["stn"] == "fused"
        for g, r in zip(got, ref):
            assert g.shape == r.shape and float((g - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max()))
        # the refused trunk on the same inputs: bit-equal to the model's own operators
        xr = x
        g_f, _ = p._trunk("encoder", xr, got[1], got[2])
        rows = ops.pn_transform(xr, got[1], _pad4(3))
        h = ops.fc_block(rows, _first_layer(enc.conv1, _pad4(3)), enc.bn1, relu=True, training=False)
        h = ops.pn_transform(h.view(B, N, 64), got[2], 64)
        g_e = ops.pn_trunk(h, B, N, [(enc.conv2, enc.bn2)], (enc.conv3, enc.bn3), False, False)
        assert torch.equal(g_f, g_e)
        # ... and on the snapshot, not the live model
        first = got[0].clone()
        for prm in enc.conv3.parameters():
            prm.mul_(1.5)
        assert torch.equal(p(x), first)


# ------------------------------------------------------------------------------------------------ contract
def test_forward_only_and_side_effect_free():
    from pnpp_hip.inference import Predictor
    B, N = 32, 1024
    model, _ = _pointnet(True)
    model.train()   # a Predictor evaluates in eval mode whatever mode the model is left in, and must not touch its statistics
    before = {k: v.clone() for k, v in model.state_dict().items()}
    p = Predictor(model)
    x = _cloud(B, N, 3, seed=4).cuda()
    outs = [[t.clone() for t in p(x, return_transforms=True)] for _ in range(3)]
    torch.cuda.synchronize()
    mem = []
    for _ in range(2):
        p(x)
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
    assert model.training and mem[0] == mem[1], mem
    after = model.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    for a, b in zip(outs[0], outs[2]):
        assert torch.equal(a, b) and not a.requires_grad
    xg = x.clone().requires_grad_(True)
    assert not p(xg).requires_grad
    # what is held between calls: folded weights, the model copy, O(B * N / 32 * 1024) partial maxima -- nothing per point and channel
    params = sum(t.numel() * t.element_size() for t in list(model.parameters()) + list(model.buffers()))
    held = p.held_tensors()
    biggest = max(t.numel() * t.element_size() for t in held)
    print(f"  persistent {p.persistent_bytes()} bytes (model {params}); largest single tensor {biggest} bytes")
    assert biggest < B * N * 128 * 4
    partials = 3 * (B * (N // 32) * 1024 * 4 + 256) + B * 3 * 64 * 64 * 2
    assert p.persistent_bytes() <= 3 * params + partials + 3 * B * 1024 * 4 + 4096
    # global_feat=False additionally holds the 64-wide point features it returns
    enc, _ = _encoder(global_feat=False, feature_transform=True, channel=6)
    pe = Predictor(enc)
    pe(torch.randn(B, 6, N, device="cuda"))
    big = max(t.numel() * t.element_size() for t in pe.held_tensors())
    assert big <= B * N * 64 * 4 < B * N * 128 * 4


def test_largest_allocation_of_a_call():
    """bytes: the largest single buffer allocated for PointNet at 32 x 1024 stays below one B*N x 128 float32 tensor"""
    from pnpp_hip.inference import Predictor
    B, N = 32, 1024
    model, _ = _pointnet(True)
    x = _cloud(B, N, 3, seed=6).cuda()
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
    print(f"  largest torch.empty of construction + one call: {max(sizes)} bytes; peak above the baseline {peak} bytes")
    assert max(sizes) < B * N * 128 * 4
    assert peak < B * N * 128 * 4   # all of a call's allocations together


def test_refresh_after_a_training_step():
    from pnpp_hip import ops
    from pnpp_hip.inference import Predictor
    B, N = 32, 1024
    model, _ = _pointnet(True)
    p = Predictor(model)
    x = _cloud(B, N, 3, seed=8)
    xg = x.cuda()
    first = p(xg).clone()
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    out = model(xg)
    ops.mse_rows(out, torch.zeros(B, 3, device="cuda")).mean().backward()
    opt.step()
    model.eval()
    torch.cuda.synchronize()
    stale = p(xg)
    assert torch.equal(first, stale), "a Predictor is a snapshot"
    with torch.no_grad():
        now = model(xg)
    assert float((stale - now).abs().max()) > 1e-6, "the training step did not move the model"
    p.refresh()
    fresh = p(xg)
    ref = pointnet64(_p64(_state(model)), x.double(), True)[0]
    _gate_eval(fresh, ref, "after refresh")
    print(f"  |predictor - model.eval()| after refresh = {float((fresh - now).abs().max()):.3e}")
