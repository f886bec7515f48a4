"""GPU parity of the single-view launch (csrc/view_kernels.hip) against its CPU restatement (tests/view_ref.py).

Bar: xyz_out, lengths_out and index bit-equal -- the zero padding included -- to the restatement handed the device's own params: the
restatement computes (v, r, u) separately in float64, holds them to one float32 spacing of what the device reports and projects on the
device's v; everything after that is IEEE float32 operations in a fixed order, integer cells and order-free maxima."""
import numpy as np
import pytest
import torch

import view_ref as vr

pytestmark = pytest.mark.gpu

SEED, STREAM = 20250917, vr.STREAM_BASE | 1
F32 = np.float32
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]        # wave, tile and scan-carry edges
GRIDS = [1, 2, 16, 32, 128]
SHAPES = [(3, 1), (6, 1), (3, 3), (6, 3)]                                # (C, B)


@pytest.fixture(scope="module")
def ops():
    from pnpp_hip import ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return ops


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _dev_lengths(lengths):
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()


def _check(ops, x, lengths=None, seed=SEED, stream=STREAM, view_dirs=None, angles=None, **kw):
    """One launch against the restatement, bit for bit; -> (out, kept, index, params) as numpy."""
    x = np.ascontiguousarray(x, F32)
    B, N, _ = x.shape
    given = {} if view_dirs is None else {"view_dirs": torch.from_numpy(np.asarray(view_dirs, F32)).cuda()}
    if angles is not None:
        given = {"angles": torch.from_numpy(np.asarray(angles, F32)).cuda()}
    xd = torch.from_numpy(x).cuda()
    out, kept, params, idx = ops.view_clouds(xd, seed, stream, lengths=_dev_lengths(lengths), index=True, **given, **kw)
    assert out.shape == x.shape and out.data_ptr() != xd.data_ptr() and kept.dtype == idx.dtype == torch.int32
    out, kept, params, idx = _np(out), _np(kept), _np(params), _np(idx)
    v, r, u = vr.basis_of(seed, stream, B, kw.get("elevation", vr.ELEVATION), view_dirs, angles, params=params)
    ref = vr.view(x, v, r, u, seed, stream, lengths, kw.get("resolution"), kw.get("splat", 1), kw.get("thickness", 0.1),
                  kw.get("drop", 0.0), kw.get("min_keep", 1))
    assert _same(kept, ref[1]), (kept, ref[1])
    assert _same(idx, ref[2])
    assert _same(out, ref[0])
    assert _same(params[:, 5], ref[3]) and _same(params[:, 6], ref[1].astype(F32)) and _same(params[:, 7], ref[4].astype(F32))
    assert _same(_np(xd), x)                                                   # out of place
    return out, kept, idx, params


def _cloud(rng, B, N, C):
    x = rng.standard_normal((B, N, C)).astype(F32)
    x[..., :3] /= np.maximum(np.linalg.norm(x[..., :3], axis=-1, keepdims=True), 1e-3).astype(F32)   # a shell: something to hide
    return x


@pytest.mark.parametrize("N", SIZES)
def test_size_grid_bit_equal(ops, N):
    """Every G x splat at this N, the four (C, B) shapes in turn; B = 3 alternates uniform and ragged (lengths 1, N and one
    between, NaN in the padding)."""
    rng = np.random.default_rng(N)
    turn = SIZES.index(N)
    for gi, G in enumerate(GRIDS):
        for splat in (0, 1, 2):
            C, B = SHAPES[(turn + gi + splat) % 4]
            x = _cloud(rng, B, N, C)
            lengths = None
            if B == 3 and (gi + turn) % 2:
                lengths = [1, N, max(1, (2 * N) // 3)]
                for b, n in enumerate(lengths):
                    x[b, n:] = np.nan
            out, kept, idx, params = _check(ops, x, lengths, resolution=G, splat=splat, stream=STREAM + gi)
            assert (kept >= 1).all() and not np.isnan(out).any() and np.isfinite(params).all()


def test_many_clouds_one_launch(ops):
    x = _cloud(np.random.default_rng(65), 65, 300, 3)
    lengths = [1 + (37 * b) % 300 for b in range(65)]
    out, kept, idx, params = _check(ops, x, lengths)                            # resolution None: ceil(sqrt(300)) = 18
    assert len({p.tobytes() for p in params[:, :3]}) == 65                      # every cloud its own direction
    th, el = params[:, 3].astype(np.float64), params[:, 4].astype(np.float64)
    assert (th >= 0).all() and (th <= 2 * np.pi).all() and (el >= vr.ELEVATION[0] - 1e-6).all() and (el <= vr.ELEVATION[1]).all()


def test_integer_lattice_equal_depths_and_cell_borders(ops):
    g = np.arange(8, dtype=F32)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, 512, 3)
    x = np.repeat(lat, 6, 0)
    dirs = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 1, 1]], F32)
    for G, splat in ((7, 0), (8, 1), (16, 2)):                                 # 7 cells over an extent of 7: every point on a border
        out, kept, idx, params = _check(ops, x, view_dirs=dirs, resolution=G, splat=splat, thickness=0.0)
        assert (kept[:5] == 64).all()                                          # an axis view at thickness 0: exactly the front layer
    front = out[0, :64]
    assert (front[:, 2] == 7).all() and np.array_equal(params[0, :3], np.array([0, 0, 1], F32))
    _check(ops, x, resolution=16)                                              # drawn directions over the same lattice


def test_identical_points_and_edge_on_plane(ops):
    same = np.tile(np.array([0.3, -1.5, 2.0], F32), (2, 100, 1))
    out, kept, idx, params = _check(ops, same, resolution=16)
    assert (kept == 100).all() and (params[:, 5] == 0).all() and _same(out, same)   # ext == 0: one cell, everything at its front
    rng = np.random.default_rng(8)
    plane = np.zeros((4, 500, 3), F32)
    plane[..., 0], plane[..., 2] = rng.uniform(-1, 1, (4, 500)), rng.uniform(-1, 1, (4, 500))
    angles = np.array([[0.0, 0.0], [0.7, 0.0], [np.pi / 2, 0.0], [3.0, 0.0]], F32)   # elevation 0: the viewer lies in the plane y = 0
    out, kept, idx, params = _check(ops, plane, angles=angles, resolution=32, thickness=0.05)
    assert (kept >= 1).all() and (kept < 250).all()                            # a line of cells: only its front edge is seen
    assert _same(params[:, 3:5], angles)
    _check(ops, plane, angles=np.array([[0.0, np.pi / 2]] * 4, F32), resolution=32)   # from straight above: t = fl(x 0 + z 1)


def test_ragged_lengths_and_nan_padding(ops):
    N = 700
    lengths = [1, N, 2, 699, 350, 0, 5000]                                      # 0 and 5000 are clamped into 1..N on the device
    x = _cloud(np.random.default_rng(9), len(lengths), N, 6)
    for b, n in enumerate(lengths):
        x[b, min(max(n, 1), N):] = np.nan
    out, kept, idx, params = _check(ops, x, lengths, resolution=24)
    assert kept[0] == 1 and kept[2] >= 1 and kept[5] == 1 and not np.isnan(out).any()
    full, *_ = _check(ops, x[1:2], None, resolution=24)
    assert not _same(full, out[1:2])                                            # cloud 0 of that launch draws another direction ...
    ang = params[1:2, 3:5]
    a, *_ = _check(ops, x[1:2], None, angles=ang, resolution=24)
    b, *_ = _check(ops, x[:2], lengths[:2], angles=params[:2, 3:5], resolution=24)
    assert _same(a[0], b[1])                                                    # ... and from the same one sees the same rows


def test_view_from_above_keeps_the_top_shell(ops):
    rng = np.random.default_rng(10)
    x = rng.uniform(-1, 1, (2, 2048, 3)).astype(F32)
    x[..., 1] *= 0.5                                                            # a slab 2 x 1 x 2
    up = np.array([[0, 1, 0], [0, 2.5, 0]], F32)
    out, kept, idx, params = _check(ops, x, view_dirs=up, resolution=16, thickness=0.1)
    assert np.array_equal(params[:, :3], np.array([[0, 1, 0], [0, 1, 0]], F32)) and np.allclose(params[:, 4], np.pi / 2)
    for b in range(2):
        k = kept[b]
        assert 0 < k < 700
        assert out[b, :k, 1].min() > 0.1                                        # within 0.1 x 2 of a neighbourhood's top, itself above 0.3
        gone = np.setdiff1d(np.arange(2048), idx[b, :k])
        assert set(np.nonzero(x[b, :, 1] < 0.1)[0]) <= set(gone)                 # everything below the top shell goes


def test_floor_passes_a_cloud_through(ops):
    x = _cloud(np.random.default_rng(11), 3, 600, 6)
    lengths = [600, 450, 600]
    x[1, 450:] = np.nan
    _, kept0, _, _ = _check(ops, x, lengths, resolution=24)
    floor = int(kept0.min()) + 1                                                # above the smallest survivor count, below the others?
    out, kept, idx, params = _check(ops, x, lengths, resolution=24, min_keep=floor)
    low = kept0 < floor
    assert low.any() and _same(params[:, 7], low.astype(F32))
    for b in np.nonzero(low)[0]:
        assert kept[b] == lengths[b] and _same(out[b, :kept[b]], x[b, :kept[b]]) and not out[b, kept[b]:].any()
        assert (idx[b, :kept[b]] == np.arange(kept[b])).all()
    assert _same(kept[~low], kept0[~low])
    out, kept, idx, params = _check(ops, x, lengths, resolution=24, min_keep=600)   # above every count, and above cloud 1's length
    assert params[:, 7].all() and kept.tolist() == lengths
    out, kept, idx, params = _check(ops, x, lengths, resolution=24, min_keep=0)
    assert not params[:, 7].any()


def test_thinning(ops):
    x = _cloud(np.random.default_rng(12), 8, 1500, 3)
    plain = _check(ops, x, resolution=32)
    zero = _check(ops, x, resolution=32, drop=0.0)
    assert all(_same(a, b) for a, b in zip(plain, zero))                        # drop = 0 is the call without drop
    out, kept, idx, params = _check(ops, x, resolution=32, drop=0.9)            # _check: the survivors are the restatement's words'
    assert (kept <= plain[1]).all() and (kept < plain[1]).any() and _same(params[:, :6], plain[3][:, :6])
    ratio = 0.9 * vr.cloud_words(SEED, STREAM, 8)[2].astype(np.float64) / 2.0 ** 32
    share = 1.0 - kept / plain[1]
    print("thinning: ratio drawn", np.round(ratio, 3), "share removed", np.round(share, 3))
    assert np.abs(share - ratio).max() <= 5 * np.sqrt(0.25 / plain[1].min())    # a binomial share of the visible points
    for b in range(8):
        assert set(idx[b, :kept[b]]) <= set(plain[2][b, :plain[1][b]])


def test_determinism_and_streams(ops):
    from pnpp_hip.augment import Augment
    from pnpp_hip.views import SingleView
    x = torch.from_numpy(_cloud(np.random.default_rng(13), 4, 900, 3)).cuda()
    run = lambda stream: ops.view_clouds(x, SEED, stream, drop=0.5, index=True)
    a, b, other = run(STREAM), run(STREAM), run(STREAM + 1)
    assert all(_same(_np(s), _np(t)) for s, t in zip(a, b))
    assert not _same(_np(a[0]), _np(other[0])) and not _same(_np(a[2]), _np(other[2]))
    sv = SingleView(seed=SEED, drop=0.5)
    o1, l1, i1 = sv.view(x, index=True)
    assert sv.draws == 1 and _same(_np(o1), _np(a[0])) and _same(_np(l1), _np(a[1])) and _same(_np(i1), _np(a[3]))
    assert _same(_np(sv.last_params), _np(a[2]))
    o2, l2 = sv(x)
    assert sv.draws == 2 and _same(_np(o2), _np(other[0])) and not _same(_np(o2), _np(o1))   # consecutive calls differ
    aug = Augment(seed=SEED)
    aug(x, kinds=())
    assert not np.array_equal(vr.cloud_words(SEED, 1, 4)[0], vr.cloud_words(SEED, STREAM, 4)[0])
    th = _np(aug.last_params)[:, 3]
    assert not _same(th, _np(a[2])[:, 3])                                       # Augment's call 1 and the view's call 1: other words


def test_resample_is_the_draw_applied_by_hand(ops):
    from pnpp_hip.views import RESAMPLE_BASE, SingleView
    x = torch.from_numpy(_cloud(np.random.default_rng(14), 5, 1000, 3)).cuda()
    lengths = torch.tensor([1000, 40, 700, 1000, 3], dtype=torch.int32).cuda()
    ragged, resampled = SingleView(seed=SEED, resolution=24), SingleView(seed=SEED, resolution=24, resample=256)
    for call in (1, 2):
        out, kept = ragged.view(x, lengths)
        got = resampled.view(x, lengths)
        assert got.shape == (5, 256, 3) and _same(_np(resampled.last_params), _np(ragged.last_params))
        want = ops.subsample_points(SEED, RESAMPLE_BASE | call, out, kept, 256)
        assert _same(_np(got), _np(want))
    k = _np(kept)
    assert k[1] <= 40 and k[4] <= 3 and (k[[0, 3]] > 256).all()                  # with and without replacement
    rows = {r.tobytes() for r in _np(out)[1, :k[1]]}
    assert all(r.tobytes() in rows for r in _np(got)[1])                        # every drawn row is a survivor


def test_capturable(ops):
    from pnpp_hip.views import SingleView
    rng = np.random.default_rng(15)
    data = [_cloud(rng, 3, 1100, 6) for _ in range(2)]
    x = torch.from_numpy(data[0]).cuda()
    lens = torch.tensor([1100, 500, 1], dtype=torch.int32).cuda()
    call = lambda: ops.view_clouds(x, SEED, STREAM, lengths=lens, resolution=128, splat=2, index=True)   # 64 KiB of LDS
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = [_np(t) for t in call()]                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    replays = []
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replays.append([_np(t).copy() for t in out])
    assert all(_same(a, b) for a, b in zip(replays[0], replays[1])) and all(_same(a, b) for a, b in zip(replays[0], want))
    x.copy_(torch.from_numpy(data[1]).cuda())
    lens.copy_(torch.tensor([7, 1100, 1099], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    fresh = ops.view_clouds(x, SEED, STREAM, lengths=lens, resolution=128, splat=2, index=True)
    assert all(_same(_np(a), _np(b)) for a, b in zip(out, fresh))               # new contents, nothing baked in


def _bank(seed=11):
    import dataloader_common as dc
    rng = np.random.default_rng(6)
    clouds = [_cloud(rng, 1, 300 + 40 * i, 3)[0] for i in range(6)]
    return dc.DeviceCloudBank(clouds, "cuda", seed=seed)


def test_bank_loader_without_a_view_is_todays(ops):
    import dataloader_common as dc
    mu = torch.arange(6, dtype=torch.float32)
    got = list(dc.BankLoader(_bank(), [mu], 128, 4, True, seed=12, view=None))
    bank = _bank()
    order = torch.randperm(6, generator=torch.Generator().manual_seed(12))
    assert len(got) == 2 and all(len(b) == 2 for b in got)
    for i, (xyz, m) in enumerate(got):
        ids = order[4 * i:4 * i + 4]
        assert _same(_np(xyz), _np(bank.sample(ids.cuda(), 128))) and _same(_np(m), mu[ids].numpy())
    assert bank.draws == 2


def test_bank_loader_with_a_view_is_draw_then_view(ops):
    import dataloader_common as dc
    from pnpp_hip.augment import Augment
    from pnpp_hip.views import STREAM_BASE, RESAMPLE_BASE, SingleView
    mu = torch.arange(6, dtype=torch.float32)
    order = torch.randperm(6, generator=torch.Generator().manual_seed(12))
    view = SingleView(seed=SEED, resolution=16, resample=128)
    got = list(dc.BankLoader(_bank(), [mu], 128, 4, True, seed=12, view=view))
    bank = _bank()
    for i, (xyz, m) in enumerate(got):
        ids = order[4 * i:4 * i + 4]
        draw = bank.sample(ids.cuda(), 256)                                     # view_points defaults to 2 num_points
        out, kept, _ = ops.view_clouds(draw, SEED, STREAM_BASE | (i + 1), resolution=16)
        assert _same(_np(xyz), _np(ops.subsample_points(SEED, RESAMPLE_BASE | (i + 1), out, kept, 128))) and xyz.shape == (len(ids), 128, 3)
        assert _same(_np(m), mu[ids].numpy())
    assert view.draws == 2
    view, aug = SingleView(seed=SEED, resolution=16), Augment(seed=SEED)        # ragged, and augmented with the lengths
    got = list(dc.BankLoader(_bank(), [mu], 128, 4, True, seed=12, view=view, view_points=200, augment=aug, kinds=("angle",)))
    bank = _bank()
    for i, batch in enumerate(got):
        assert len(batch) == 3
        ids = order[4 * i:4 * i + 4]
        out, kept, _ = ops.view_clouds(bank.sample(ids.cuda(), 200), SEED, STREAM_BASE | (i + 1), resolution=16)
        want, (wmu,), _ = ops.augment_clouds(out, SEED, (1 << 63) | (i + 1), [mu[ids].cuda()], ["angle"], lengths=kept)
        assert _same(_np(batch[0]), _np(want)) and _same(_np(batch[1]), _np(wmu)) and _same(_np(batch[2]), _np(kept))
        k = _np(kept)
        assert all(not _np(batch[0])[b, k[b]:].any() for b in range(len(ids)))  # the padding stays exact zeros through the augmentation


def test_training_step_on_the_ragged_result(ops):
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    from pnpp_hip.views import SingleView
    torch.manual_seed(0)
    model = PointNetPPVonMises(sampler="device").cuda().train()
    x = torch.from_numpy(_cloud(np.random.default_rng(16), 4, 2048, 3)).cuda()
    view = SingleView(seed=SEED, min_keep=model.sa1.min_length())
    seen, lengths = view(x)
    k = _np(lengths)
    assert (k >= model.sa1.min_length()).all() and (k < 2048).any()
    mu_gt, kappa_gt = torch.zeros(4).cuda(), torch.ones(4).cuda()
    loss = ops.vm_head_kl_loss(model.features(seen, lengths=lengths), mu_gt, kappa_gt)
    loss.backward()
    assert torch.isfinite(loss).item()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) > 10 and all(torch.isfinite(g).all().item() for g in grads) and any(float(g.abs().max()) > 0 for g in grads)


@pytest.mark.parametrize("name,ckpt", [("train_single_peak_vonMises_KL", "vonMises_best.pth"),
                                       ("train_multi_peaks_vonMises_KL", "mvM_best.pth"), ("train_8dir_KL", "8dir_KLdiv_0926.pth")])
def test_scripts_train_with_views(name, ckpt, tmp_path, monkeypatch):
    """--views --synthetic through the scripts' own loop: the train split goes through ViewLoader, its batches keep the uniform shape
    (so the step is still captured), the losses are finite numbers."""
    import importlib
    from pnpp_hip import trainer
    mod = importlib.import_module(name)
    monkeypatch.setattr(mod, "RES", tmp_path)
    monkeypatch.setattr(mod, "FIGS", tmp_path / "figs")
    monkeypatch.setattr(mod, "EPOCHS", 2)
    monkeypatch.setattr(mod, "BATCH", 16)
    monkeypatch.setattr(mod, "NUM_POINTS", 256)
    seen = []
    real = trainer.ViewLoader.__iter__

    def spy(self):
        for batch in real(self):
            seen.append((self.view.draws, tuple(batch[0].shape[1:]), self.view.last_params[:, 6].clone()))
            yield batch

    monkeypatch.setattr(trainer.ViewLoader, "__iter__", spy)
    hist, test_loss = mod.main(["--synthetic", "64", "--sampler", "device", "--views"])
    train = hist["total"]["train"] if "total" in hist else hist["train"]
    assert len(train) == 2 and all(v == v and 0 < v < 20.0 for v in train) and test_loss == test_loss
    assert (tmp_path / ckpt).exists()
    steps = hist["_trainer"]["steps"] if "_trainer" in hist else hist["steps"]
    assert steps["graph"] >= 1                                                     # the loader runs outside the captured step
    assert [d for d, _, _ in seen] == list(range(1, 7))                            # 44 train clouds: 3 batches x 2 epochs, all viewed
    assert all(shape == (256, 3) for _, shape, _ in seen)
    assert all(float(k.max()) < 256 and float(k.min()) >= 1 for _, _, k in seen)   # one side of each cloud, resampled to NUM_POINTS
