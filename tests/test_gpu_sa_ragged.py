"""Ragged batches of the PointNet++ models on the GPU: a padded (B,N,3) tensor plus per-cloud lengths through the four index kernels
that read the cloud itself (kNN, farthest-point sampling, radius query, random centre draw), the two paired launches that carry them,
the models and the Predictors.

Two yardsticks throughout: the C oracle on the sliced cloud xyz[b, :len], or the uniform kernel on that slice alone.  Index results are
compared bit for bit.  A model in train mode is compared, bit for bit, with the uniform call on the FAR-PADDED batch: every padding
row replaced by a point at 100 x the batch's largest coordinate magnitude -- once no such point enters a neighbour list of the uniform
search (checked on the CPU with the oracle: a condition on the inputs), both calls run the same launches on the same lists.  Eval-mode
outputs are held to the gates the existing inference tests apply (imported from them)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import has_gpu
from test_gpu_inference import _gate_eval, _randomise
from test_gpu_pointnet_pp_cls import _gate as _gate_cls

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an AMD GPU")]

LENS_TWO_TILES = [1100, 1025, 1024, 1023, 257, 256, 129, 128, 65, 64, 33, 32]     # N = 1100: KNN_TILE = 1024, two tiles
LENS_ONE_TILE = [300, 299, 257, 256, 255, 129, 128, 32]                            # N = 300
SHAPES = {1100: LENS_TWO_TILES, 300: LENS_ONE_TILE}
K = 32
SEED, STREAM = 0x1234ABCD5678, 77


@pytest.fixture(scope="module")
def ops():
    from pnpp_hip import ops
    return ops


_clouds = {}


def clouds(oracle, B, N):
    """synthetic clouds, computed once per shape and never written to"""
    key = (B, N)
    if key not in _clouds:
        _clouds[key] = oracle.synthetic_clouds(B, N, seed=1234 + N)[0]
    return _clouds[key]


def dev_lengths(lens):
    return torch.tensor(lens, dtype=torch.int32).cuda()


def refill(xyz, lens, rows):
    """a copy of xyz whose padding rows (>= len) are overwritten with rows[b] cycled"""
    out = xyz.clone()
    for b, n in enumerate(lens):
        pad = out.shape[1] - n
        if pad:
            r = rows[b]
            out[b, n:] = r[torch.arange(pad) % r.shape[0]]
    return out


def far_padded(xyz, lens):
    far = 100.0 * float(xyz.abs().max())
    return refill(xyz, lens, [torch.full((1, 3), far)] * len(lens))


def queries(xyz):
    """S = 8 explicit queries per cloud that are no points of it: midpoints of rows of every cloud's valid part"""
    return (0.5 * (xyz[:, 0:8] + xyz[:, 8:16])).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# kNN
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1100, 300])
def test_knn_rows_equal_the_search_on_the_slice(ops, oracle, N):
    lens = SHAPES[N]
    xyz = clouds(oracle, len(lens), N)
    q = queries(xyz)
    got = ops.knn(q.cuda(), xyz.cuda(), K, lengths=lens).cpu()
    for b, n in enumerate(lens):
        sl = xyz[b:b + 1, :n].contiguous()
        assert int(got[b].max()) < n
        assert torch.equal(got[b:b + 1].long(), oracle.knn_indices(q[b:b + 1], sl, K)), f"cloud {b} (len {n}) against the oracle"
        assert torch.equal(got[b:b + 1], ops.knn(q[b:b + 1].cuda(), sl.cuda(), K).cpu()), f"cloud {b} (len {n}) against the uniform kernel"
    # the padding rows hold anything: the queries themselves (closer than any real point), or far-away values
    for what, rows in (("copies of the queries", list(q)), ("other finite values", [torch.randn(7, 3) * 50 for _ in lens])):
        again = ops.knn(q.cuda(), refill(xyz, lens, rows).cuda(), K, lengths=dev_lengths(lens)).cpu()
        assert torch.equal(again, got), what


def test_knn_cloud_shorter_than_k_repeats_slot_zero(ops, oracle):
    """k > lengths[b] cannot be refused on the device (the host refuses it where it sees the lengths): at kernel level the slots
    >= len repeat slot 0, so no index >= len is ever written"""
    N, short = 300, 20
    xyz = clouds(oracle, len(LENS_ONE_TILE), N)[:2].contiguous()
    q = queries(xyz)
    with pytest.raises(ValueError, match=r"lengths\[0\] = 20"):
        ops.knn(q.cuda(), xyz.cuda(), K, lengths=[short, N])
    got = ops.knn(q.cuda(), xyz.cuda(), K, lengths=dev_lengths([short, N])).cpu()
    assert int(got[0].max()) < short
    assert torch.equal(got[0, :, :short].long(), oracle.knn_indices(q[:1], xyz[:1, :short].contiguous(), short)[0])
    assert torch.equal(got[0, :, short:], got[0, :, :1].expand(-1, K - short))
    assert torch.equal(got[1:].long(), oracle.knn_indices(q[1:], xyz[1:], K))


# ------------------------------------------------------------------------------------------------------------------------------
# the pair launch
# ------------------------------------------------------------------------------------------------------------------------------
def _knn_pair(lib, ops, xyz, c1, c2, k1, k2, lengths):
    B, N, _ = xyz.shape
    S1, S2 = c1.shape[1], c2.shape[1]
    idx1 = torch.empty(B, S1, k1, dtype=torch.int32, device="cuda")
    idx2 = torch.empty(B, S2, k2, dtype=torch.int32, device="cuda")
    nx1 = torch.empty(B, S1, 3, device="cuda")
    nx2 = torch.empty(B, S2, 3, device="cuda")
    mom = torch.zeros(lib.pnpp_knn_pair_partials(B, S1, N), 16, dtype=torch.float64, device="cuda")
    from pnpp_hip import _lib
    if lengths is None:
        _lib.check(lib.pnpp_knn_pair(xyz.data_ptr(), B, N, c1.data_ptr(), S1, k1, idx1.data_ptr(), nx1.data_ptr(), c2.data_ptr(), S2, k2,
                                     idx2.data_ptr(), nx2.data_ptr(), mom.data_ptr(), ops._stream()))
    else:
        _lib.check(lib.pnpp_knn_pair_ragged(xyz.data_ptr(), B, N, lengths.data_ptr(), c1.data_ptr(), S1, k1, idx1.data_ptr(), nx1.data_ptr(),
                                            c2.data_ptr(), S2, k2, idx2.data_ptr(), nx2.data_ptr(), mom.data_ptr(), ops._stream()))
    return idx1, nx1, idx2, nx2, mom[:, :9].clone()


def _saved_neighbours(ops, pre, B, N, S, k, D, channels):
    from pnpp_hip import _lib
    d = ops._sa_desc(B, N, S, k, D, channels, False, True, 1e-5, 0.1)
    off = _lib.lib().pnpp_sa_saved_neighbours(C.byref(d), pre["saved"].data_ptr()) - pre["saved"].data_ptr()
    return pre["saved"][off:off + 4 * B * S * k].view(torch.int32).view(B, S, k)


@pytest.mark.parametrize("N", [1100, 300])
def test_pair_launch(ops, oracle, N):
    from pnpp_hip import _lib
    from models.pointnet_pp_8dir import PointNetSetAbstraction
    lib = _lib.lib()
    lens = [n for n in SHAPES[N] if n >= 128]
    B, S1, S2 = len(lens), 128, 32
    xyz = clouds(oracle, len(SHAPES[N]), N)[:B].contiguous()
    L = dev_lengths(lens)
    xg = xyz.cuda()
    c1 = ops.sample_random(SEED, STREAM, B, N, S1, "cuda", lengths=L)
    c2 = ops.sample_random(SEED, STREAM + 1, B, S1, S2, "cuda")
    idx1, nx1, idx2, nx2, mom = _knn_pair(lib, ops, xg, c1, c2, K, K, L)
    # both levels against the two separate searches
    new1 = ops.index_points(xg, c1)
    new2 = ops.index_points(new1, c2)
    assert torch.equal(nx1, new1) and torch.equal(nx2, new2)
    assert torch.equal(idx1, ops.knn(new1, xg, K, lengths=L)) and int(idx1.max(-1)[0].max(-1)[0].sub(L).max()) < 0
    assert torch.equal(idx2, ops.knn(new2, new1, K))
    # the training entry point (ops.group_pair) writes the same lists and centres into the levels' workspaces
    sa1 = PointNetSetAbstraction(S1, K, 0, [64, 64, 128])
    sa2 = PointNetSetAbstraction(S2, K, 128, [128, 128, 256])
    pre1, pre2 = ops.group_pair(xg, c1, c2, K, sa1.convs, K, sa2.convs, lengths=lens)
    assert torch.equal(_saved_neighbours(ops, pre1, B, N, S1, K, 0, [64, 64, 128]), idx1)
    assert torch.equal(_saved_neighbours(ops, pre2, B, S1, S2, K, 128, [128, 128, 256]), idx2)
    assert torch.equal(pre1["new_xyz"], nx1) and torch.equal(pre2["new_xyz"], nx2)
    # level 1's moment partials: those of the uniform pair call on the far-padded batch, bit for bit
    far = far_padded(xyz, lens)
    ref1 = oracle.knn_indices(oracle.index_points(far, c1.cpu().long()), far, K)
    assert bool((ref1 < torch.tensor(lens).view(B, 1, 1)).all()), "input condition: a far point entered a neighbour list"
    u1, _, u2, _, umom = _knn_pair(lib, ops, far.cuda(), c1, c2, K, K, None)
    assert torch.equal(u1, idx1) and torch.equal(u2, idx2)
    assert torch.equal(mom, umom) and bool(mom.abs().sum() > 0)


# ------------------------------------------------------------------------------------------------------------------------------
# farthest-point sampling, radius query
# ------------------------------------------------------------------------------------------------------------------------------
def _starts(lens, mult=7):
    return torch.tensor([(mult * (b + 1)) % n for b, n in enumerate(lens)])


@pytest.mark.parametrize("N", [1100, 300])
def test_fps_rows_equal_the_sampling_of_the_slice(ops, oracle, N):
    lens = SHAPES[N] + [1]                                            # npoint = 16: some clouds are shorter than that
    xyz = clouds(oracle, len(lens), N)
    start = _starts(lens)
    got = ops.farthest_point_sample(xyz.cuda(), 16, start, lengths=lens).cpu()
    for b, n in enumerate(lens):
        ref = oracle.farthest_point_sample(xyz[b:b + 1, :n].contiguous(), 16, start[b:b + 1])
        assert torch.equal(got[b:b + 1].long(), ref), f"cloud {b} (len {n})"
    again = ops.farthest_point_sample(refill(xyz, lens, [torch.randn(5, 3) * 30 for _ in lens]).cuda(), 16, start, lengths=lens).cpu()
    assert torch.equal(again, got)


def test_fps_tail_points_in_lds(ops, oracle):
    """N > 16384: the points beyond the register file live in the LDS tail; a length can end inside it, at its edge or far below"""
    N, lens = 16448, [16448, 16385, 16384, 100]
    xyz = clouds(oracle, 4, N)
    start = torch.tensor([16447, 16384, 5, 99])
    got = ops.farthest_point_sample(xyz.cuda(), 8, start, lengths=lens).cpu()
    for b, n in enumerate(lens):
        ref = oracle.farthest_point_sample(xyz[b:b + 1, :n].contiguous(), 8, start[b:b + 1])
        assert torch.equal(got[b:b + 1].long(), ref), f"cloud {b} (len {n})"


@pytest.mark.parametrize("radius,nsample", [(0.2, 32), (0.4, 64)])
def test_ball_query_rows_equal_the_query_on_the_slice(ops, oracle, radius, nsample):
    N, lens = 1100, LENS_TWO_TILES
    xyz = clouds(oracle, len(lens), N)
    L = dev_lengths(lens)
    centre = ops.farthest_point_sample(xyz.cuda(), 24, _starts(lens), lengths=L)
    new_xyz = ops.index_points(xyz.cuda(), centre)
    got = ops.ball_query(radius, nsample, xyz.cuda(), new_xyz, lengths=L).cpu()
    nx = new_xyz.cpu()
    for b, n in enumerate(lens):
        ref = oracle.ball_query(radius, nsample, xyz[b:b + 1, :n].contiguous(), nx[b:b + 1])
        assert torch.equal(got[b:b + 1].long(), ref), f"cloud {b} (len {n})"
        assert int(got[b].max()) < n
    inside = refill(xyz, lens, list(nx))                              # padding rows inside every ball
    assert torch.equal(ops.ball_query(radius, nsample, inside.cuda(), new_xyz, lengths=L).cpu(), got)


# ------------------------------------------------------------------------------------------------------------------------------
# the centre draw
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1100, 300])
def test_sample_random_rows_equal_the_uniform_draw_at_the_length(ops, N):
    from oracle import sampler
    lens = SHAPES[N]
    B, npoint = len(lens), 32
    got = ops.sample_random(SEED, STREAM, B, N, npoint, "cuda", lengths=lens).cpu().numpy()
    for b, n in enumerate(lens):
        assert np.array_equal(got[b], sampler.sample_random(SEED, STREAM, B, n, npoint)[b]), f"cloud {b} (len {n})"
    # the counter forms: the same draws, the counter advances by 1 and by 2, the second draw of a pair is uniform
    L = dev_lengths(lens)
    counter = torch.tensor([5, 0], dtype=torch.int64).cuda()
    one = ops.sample_random_dev(SEED, counter, STREAM - 5, B, N, npoint, lengths=L)
    assert counter.tolist() == [6, 0] and np.array_equal(one.cpu().numpy(), got)
    a, b2 = ops.sample_random_dev2(SEED, counter, STREAM - 6, B, N, npoint, npoint, 8, lengths=L)
    assert counter.tolist() == [8, 0] and np.array_equal(a.cpu().numpy(), got)
    assert torch.equal(b2, ops.sample_random(SEED, STREAM + 1, B, npoint, 8, "cuda"))


def test_all_lengths_equal_to_n_is_the_uniform_twin(ops, oracle):
    from pnpp_hip import _lib
    lib = _lib.lib()
    B, N = 4, 1100
    xyz = clouds(oracle, len(LENS_TWO_TILES), N)[:B].contiguous().cuda()
    full = dev_lengths([N] * B)
    q = queries(xyz)
    assert torch.equal(ops.knn(q, xyz, K, lengths=full), ops.knn(q, xyz, K))
    start = torch.tensor([0, 5, 1099, 64])
    fps = ops.farthest_point_sample(xyz, 16, start)
    assert torch.equal(ops.farthest_point_sample(xyz, 16, start, lengths=full), fps)
    new = ops.index_points(xyz, fps)
    assert torch.equal(ops.ball_query(0.2, 32, xyz, new, lengths=full), ops.ball_query(0.2, 32, xyz, new))
    c1 = ops.sample_random(SEED, STREAM, B, N, 128, "cuda")
    assert torch.equal(ops.sample_random(SEED, STREAM, B, N, 128, "cuda", lengths=full), c1)
    ca, cb = torch.zeros(2, dtype=torch.int64).cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    assert torch.equal(ops.sample_random_dev(SEED, ca, STREAM, B, N, 128, lengths=full), ops.sample_random_dev(SEED, cb, STREAM, B, N, 128))
    r1, r2 = ops.sample_random_dev2(SEED, ca, STREAM, B, N, 128, 128, 32, lengths=full)
    u1, u2 = ops.sample_random_dev2(SEED, cb, STREAM, B, N, 128, 128, 32)
    assert torch.equal(r1, u1) and torch.equal(r2, u2) and ca.tolist() == cb.tolist() == [3, 0]
    for a, b in zip(_knn_pair(lib, ops, xyz, c1, u2, K, K, full), _knn_pair(lib, ops, xyz, c1, u2, K, K, None)):
        assert torch.equal(a, b)
    from models.pointnet_pp_8dir import PointNetSetAbstraction
    sa1, sa2 = PointNetSetAbstraction(128, K, 0, [64, 64, 128]), PointNetSetAbstraction(32, K, 128, [128, 128, 256])
    levels = ((B, N, 128, K, 0, [64, 64, 128]), (B, 128, 32, K, 128, [128, 128, 256]))
    ragged = ops.group_pair(xyz, c1, u2, K, sa1.convs, K, sa2.convs, lengths=full)
    uniform = ops.group_pair(xyz, c1, u2, K, sa1.convs, K, sa2.convs)
    for a, b, level in zip(ragged, uniform, levels):
        assert torch.equal(a["new_xyz"], b["new_xyz"])
        assert torch.equal(_saved_neighbours(ops, a, *level), _saved_neighbours(ops, b, *level))
    d1 = ops._sa_desc(B, N, 128, K, 0, [64, 64, 128], False, False, 1e-5, 0.1)
    d2 = ops._sa_desc(B, 128, 32, K, 128, [128, 128, 256], False, False, 1e-5, 0.1)
    outs = []
    for lengths in (full, None):
        bufs = [torch.empty(B, 128, K, dtype=torch.int32, device="cuda"), torch.empty(B, 128, 3, device="cuda"),
                torch.empty(B, 32, K, dtype=torch.int32, device="cuda"), torch.empty(B, 32, 3, device="cuda")]
        tail = (c1.data_ptr(), u2.data_ptr(), *[t.data_ptr() for t in bufs], ops._stream())
        if lengths is None:
            _lib.check(lib.pnpp_sa_infer_group_pair(C.byref(d1), C.byref(d2), xyz.data_ptr(), *tail))
        else:
            _lib.check(lib.pnpp_sa_infer_group_pair_ragged(C.byref(d1), C.byref(d2), xyz.data_ptr(), lengths.data_ptr(), *tail))
        outs.append(bufs)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------------------------------------
MODEL_LENS = [300, 299, 257, 256, 255, 129, 128, 128]     # B = 8 from the one-tile list's lengths >= 128 (its shortest twice)


def _model_case(oracle, B=8, N=300):
    from pnpp_hip import ops, sampling
    xyz = clouds(oracle, len(LENS_ONE_TILE), N)[:B].contiguous()
    lens = MODEL_LENS[:B]
    L = dev_lengths(lens)
    torch.manual_seed(11)
    sampling.reset()
    c1, c2 = sampling.device_random_centres_pair(B, N, 128, 128, 32, "cuda", lengths=L)     # the ragged device draw
    assert bool((c1 < L.view(B, 1)).all())
    far = far_padded(xyz, lens)
    ref1 = oracle.knn_indices(oracle.index_points(far, c1.cpu().long()), far, 32)
    assert bool((ref1 < torch.tensor(lens).view(B, 1, 1)).all()), "input condition: a far point entered a neighbour list"
    return xyz.cuda(), far.cuda(), lens, L, (c1, c2)


def _vonmises_step(m, xyz, centres, lengths, oracle):
    from pnpp_hip import ops
    B = xyz.shape[0]
    _, mu_gt, kappa_gt, _ = oracle.synthetic_clouds(B, 16, seed=5)
    g = torch.Generator().manual_seed(3)
    mask = (torch.rand(B, 256, generator=g) < 0.5).to(torch.uint8).cuda()
    mu, kappa = m(xyz, centres=centres, drop_mask=mask, lengths=lengths)
    loss = ops.kl_von_mises_single(mu, kappa, mu_gt.cuda(), kappa_gt.cuda()).mean()
    loss.backward()
    return (mu, kappa), loss


def _mvm_step(m, xyz, centres, lengths, oracle):
    from pnpp_hip import ops
    import synthetic
    B = xyz.shape[0]
    fwd = oracle.synthetic_clouds(B, 16, seed=5)[3]
    g = torch.Generator().manual_seed(3)
    Kgt = torch.tensor([1, 2, 4])[torch.randint(0, 3, (B,), generator=g)]
    vm_gt = synthetic.multi_peak_gt(fwd, Kgt)
    masks = [(torch.rand(B, w, generator=g) < 0.6).to(torch.uint8).cuda() for w in (512, 256)]
    out = m(xyz, centres=centres, drop_masks=masks, lengths=lengths)
    loss = ops.match_loss(*out, vm_gt.cuda(), Kgt.cuda()).mean()
    loss.backward()
    return out, loss


def _train_models():
    from models.pointnet_pp_mvM import PointNetPPMvM
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    return {"vonmises": (PointNetPPVonMises, _vonmises_step), "mvm": (PointNetPPMvM, _mvm_step)}


@pytest.mark.parametrize("which", ["vonmises", "mvm"])
def test_training_step_equals_the_uniform_step_on_the_far_padded_batch(oracle, which):
    cls, step = _train_models()[which]
    xyz, far, lens, L, centres = _model_case(oracle)
    torch.manual_seed(42)
    m = cls(sampler="device")
    if which == "mvm":
        with torch.no_grad():     # off the zero-initialised pi / mu heads (every angle the degenerate fallback)
            m.head_pi.weight.normal_(0, 0.05)
            m.head_mu.weight.normal_(0, 0.05)
            m.head_mu.bias.normal_(0, 0.05)
    ragged, uniform = m.cuda().train(), copy.deepcopy(m).cuda().train()
    out_r, loss_r = step(ragged, xyz, centres, lens, oracle)
    out_u, loss_u = step(uniform, far, centres, None, oracle)
    for i, (a, b) in enumerate(zip(out_r, out_u)):
        assert torch.equal(a, b), f"output {i}"
    assert torch.equal(loss_r, loss_u) and bool(torch.isfinite(loss_r))
    for (name, p), q in zip(ragged.named_parameters(), uniform.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), name
    for (name, p), q in zip(ragged.named_buffers(), uniform.buffers()):
        assert torch.equal(p, q), name


def _eval_models():
    from models.pointnet_pp_8dir import PointNetPP8Dir
    from models.pointnet_pp_mvM import PointNetPPMvM
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    return {"vonmises": PointNetPPVonMises, "mvm": PointNetPPMvM, "8dir": PointNetPP8Dir}


def _tuple(t):
    return t if isinstance(t, (tuple, list)) else (t,)


@pytest.mark.parametrize("which", ["vonmises", "mvm", "8dir"])
def test_eval_and_predictor(oracle, which):
    from pnpp_hip.inference import Predictor
    cls = _eval_models()[which]
    xyz, far, lens, L, centres = _model_case(oracle)
    torch.manual_seed(3)
    m = _randomise(cls(sampler="device"), 103).cuda().eval()
    p = Predictor(m)
    with torch.no_grad():
        got = _tuple(p(xyz, centres=centres, lengths=lens))
        assert p.last_plan["sa1"] == p.last_plan["sa2"] == p.last_plan["sa3"] == "fused"
        padded = _tuple(p(far, centres=centres))
        ev = _tuple(m(xyz, centres=centres, lengths=L))
        for i, (g, u, e) in enumerate(zip(got, padded, ev)):
            assert torch.equal(g, u), f"Predictor output {i}: ragged against far-padded"
            _gate_eval(g, e.cpu(), f"{cls.__name__} output {i}: Predictor(lengths) against model.eval()(lengths)")
        for b, n in enumerate(lens):     # each cloud alone, with its own centres
            alone = _tuple(m(xyz[b:b + 1, :n].contiguous(), centres=(centres[0][b:b + 1], centres[1][b:b + 1])))
            for i, (e, a) in enumerate(zip(ev, alone)):
                _gate_eval(e[b:b + 1], a.cpu(), f"{cls.__name__} output {i}, cloud {b} (len {n}) alone")


# ------------------------------------------------------------------------------------------------------------------------------
# the classifier
# ------------------------------------------------------------------------------------------------------------------------------
CLS_LENS = [300, 257, 256, 129, 70, 64]


def _cls_case(oracle):
    from models.pointnet_pp_cls import PointNetPlusPlusCls
    B, N = len(CLS_LENS), 300
    xyz = clouds(oracle, len(LENS_ONE_TILE), N)[:B]
    g = torch.Generator().manual_seed(9)
    normals = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1)
    x = torch.cat([xyz, normals], -1).transpose(1, 2).contiguous().cuda()          # (B, 6, N)
    start = (_starts(CLS_LENS).cuda(), _starts([64] * B, mult=5).cuda())
    torch.manual_seed(21)
    m = PointNetPlusPlusCls(num_classes=10, sa1=(64, 0.2, 32), sa2=(16, 0.4, 64))
    return m, x, start


def test_cls_eval_and_predictor_rows_equal_the_cloud_alone(oracle):
    from pnpp_hip.inference import Predictor
    m, x, start = _cls_case(oracle)
    m = _randomise(m, 31).cuda().eval()
    p = Predictor(m)
    with torch.no_grad():
        ev = m(x, start, lengths=CLS_LENS)
        pr = p(x, start, lengths=CLS_LENS)
        for b, n in enumerate(CLS_LENS):
            alone = m(x[b:b + 1, :, :n].contiguous(), (start[0][b:b + 1], start[1][b:b + 1]))
            _gate_cls(ev[b:b + 1], alone, f"model.eval() cloud {b} (len {n})")
            _gate_cls(pr[b:b + 1], alone, f"Predictor cloud {b} (len {n})")


def test_cls_training_step_equals_the_step_assembled_by_hand(oracle):
    from pnpp_hip import ops
    m, x, start = _cls_case(oracle)
    B = x.shape[0]
    model, hand = m.cuda().train(), copy.deepcopy(m).cuda().train()
    g = torch.Generator().manual_seed(4)
    masks = [(torch.rand(B, w, generator=g) < 0.6).to(torch.uint8).cuda() for w in (512, 256)]
    target = torch.randint(0, 10, (B,), generator=g).cuda()
    L = dev_lengths(CLS_LENS)

    logp = model(x, start, drop_masks=masks, lengths=CLS_LENS)
    loss = ops.nll_loss(logp, target)
    loss.backward()

    xyz, points = hand.split_input(x)
    c1 = ops.farthest_point_sample(xyz, 64, start[0], lengths=L)
    assert bool((c1 < L.view(B, 1)).all())
    nbr = ops.ball_query(0.2, 32, xyz, ops.index_points(xyz, c1), lengths=L)
    assert bool((nbr < L.view(B, 1, 1)).all())
    l1_xyz, l1_pts = ops.set_abstraction(xyz, points, c1, 32, False, True, hand.sa1.mlp_convs, hand.sa1.mlp_bns, neighbour_idx=nbr)
    l2_xyz, l2_pts = hand.sa2.rows(l1_xyz, l1_pts, start[1])
    h = hand.sa3.rows(l2_xyz, l2_pts)[1].view(B, -1)
    h = ops.fc_block(h, hand.fc1, hand.bn1, relu=True, dropout=hand.dropout1, training=True, mask=masks[0])
    h = ops.fc_block(h, hand.fc2, hand.bn2, relu=True, dropout=hand.dropout2, training=True, mask=masks[1])
    logp_h = ops.log_softmax(ops.fc_block(h, hand.fc3, training=True))
    loss_h = ops.nll_loss(logp_h, target)
    loss_h.backward()

    assert torch.equal(logp, logp_h) and torch.equal(loss, loss_h) and bool(torch.isfinite(loss))
    for (name, a), b in zip(model.named_parameters(), hand.parameters()):
        assert a.grad is not None and torch.equal(a.grad, b.grad), name


# ------------------------------------------------------------------------------------------------------------------------------
# the two samplers that draw on the host generator
# ------------------------------------------------------------------------------------------------------------------------------
def test_host_draws_are_the_per_cloud_draws_in_batch_order(oracle):
    from models.pointnet_pp_8dir import PointNetSetAbstraction
    lens = [300, 129, 64, 33]
    xyz = clouds(oracle, len(LENS_ONE_TILE), 300)[:len(lens)].contiguous().cuda()
    for sampler in ("randperm", "fps"):
        sa = PointNetSetAbstraction(16, 8, 0, [32, 32, 64], sampler=sampler)
        torch.manual_seed(5)
        batch = sa._centres(xyz, lens)
        torch.manual_seed(5)
        alone = torch.cat([sa._centres(xyz[b:b + 1, :n].contiguous()) for b, n in enumerate(lens)])
        assert torch.equal(batch.long(), alone.long()), sampler
        assert bool((batch.cpu() < torch.tensor(lens).view(-1, 1)).all())
