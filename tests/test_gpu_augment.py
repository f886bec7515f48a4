"""GPU parity of the augmentation launch (csrc/augment_kernels.hip) against its CPU restatement (tests/augment_ref.py).

Bar: bit-equal wherever the kernel's arithmetic is IEEE basic operations in a fixed order (the float32 rotation, scale, targets:
evaluated with the returned c, s, scale, because float64 cos / sin of two maths libraries may differ in the last bit before the one
rounding); one float32 ulp where float64 libm values are rounded (c, s, the jitter)."""
import math

import numpy as np
import pytest
import torch

import augment_ref as ar

pytestmark = pytest.mark.gpu

SEED, STREAM = 20240611, ar.STREAM_BASE | 1
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from pnpp_hip import ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return ops


@pytest.fixture(scope="module")
def gt():
    """64 clouds' ground truth (synthetic.py), shared and never written."""
    import synthetic
    _, mu, kappa, fwd = synthetic.rotated_clouds(64, 257, seed=5)
    K = torch.tensor([0, 1, 2, 4]).repeat(16)
    return {"mu": mu, "kappa": kappa, "fwd": fwd, "K": K, "vm3": synthetic.multi_peak_gt(fwd, K)}


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _check_params(params, B, yaw=True, scale=None):
    """The returned (B,4) against the restatement: theta and scale bit-equal, c and s one rounding of float64 cos / sin."""
    th, c, s, sc = ar.cloud_params(SEED, STREAM, B, yaw, scale)
    p = _np(params)
    assert np.abs(p[:, 0].astype(np.float64) - np.cos(th)).max() <= 2.0 ** -24
    assert np.abs(p[:, 1].astype(np.float64) - np.sin(th)).max() <= 2.0 ** -24
    assert _same(p[:, 3], th.astype(F32)) and _same(p[:, 2], sc)
    return th, p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


@pytest.mark.parametrize("N,C", [(257, 3), (1, 3), (260, 3), (257, 6), (258, 6)])   # one row past a tile; 4- and 16-byte lanes
def test_rotation_bit_equal(ops, N, C):
    g = torch.Generator().manual_seed(N * 10 + C)
    x = torch.randn(5, N, C, generator=g)
    xd = x.cuda()
    out, targets, params = ops.augment_clouds(xd, SEED, STREAM)
    assert targets == [] and out.shape == x.shape and out.data_ptr() != xd.data_ptr()
    _, c, s, sc = _check_params(params, 5)
    got = _np(out)
    assert _same(got, ar.points(x.numpy(), c, s, sc))
    assert _same(got[..., 1], x.numpy()[..., 1])
    if C == 6:
        assert _same(got[..., 4], x.numpy()[..., 4])                           # normals: rotated only, y kept
    assert _same(_np(xd), x.numpy())                                           # out of place


def test_ragged_padding_is_copied(ops, gt):
    lengths = [1, 257, 130, 0, 256]
    x = torch.randn(5, 257, 3, generator=torch.Generator().manual_seed(1))
    for b, n in enumerate(lengths):
        x[b, n:] = float("nan")
    mu = gt["mu"][:5]
    out, (mu2,), params = ops.augment_clouds(x.cuda(), SEED, STREAM, [mu.cuda()], ["angle"], lengths=torch.tensor(lengths, dtype=torch.int32).cuda())
    th, c, s, sc = _check_params(params, 5)
    got = _np(out)
    for b, n in enumerate(lengths):
        assert _same(got[b, n:], x.numpy()[b, n:])                             # NaN padding, byte for byte
    assert _same(got, ar.points(x.numpy(), c, s, sc, lengths=lengths))
    assert not np.isnan(got[1]).any() and not np.isnan(got[4, :256]).any()
    assert _same(_np(mu2), ar.shift_angles(mu.numpy(), th))                    # the empty cloud's target moves all the same
    assert _np(mu2)[3] != mu.numpy()[3]


def test_targets_bit_equal_and_geometric(ops, gt):
    from models.pointnet_pp_8dir import DIRS_8
    B = 64
    x = torch.randn(B, 3, 3, generator=torch.Generator().manual_seed(2)).cuda()
    mu, kappa, fwd, K, vm3 = (gt[k] for k in ("mu", "kappa", "fwd", "K", "vm3"))
    vm2 = torch.stack([mu, kappa], 1)
    _, (a1, a2, a3, a4), params = ops.augment_clouds(x, SEED, STREAM, [mu.cuda(), vm2.cuda(), vm3.cuda(), fwd.cuda()],
                                                     ["angle", "vm", "vm", "axis"], counts=[None, None, K.cuda(), None])
    th, c, s, _ = _check_params(params, B)
    assert _same(_np(a1), ar.shift_angles(mu.numpy(), th))                     # theta is one exact multiply: nothing returned is needed
    assert _same(_np(a2), ar.vm_table(vm2.numpy(), th))
    assert _same(_np(a3), ar.vm_table(vm3.numpy(), th, K.numpy()))
    for b in range(B):
        assert _same(_np(a3)[b, int(K[b]):], vm3.numpy()[b, int(K[b]):])       # rows at or beyond the count: the input's
    assert _same(_np(a4), ar.axes(fwd.numpy(), c, s))
    rot = _np(a4).astype(np.float64)
    assert ar.angular_distance(_np(a1), np.arctan2(rot[:, 0], -rot[:, 2])).max() <= 1e-6
    assert ar.angular_distance(_np(a3)[:, 0, 0][_np(K) > 0], np.arctan2(rot[:, 0], -rot[:, 2])[_np(K) > 0]).max() <= 1e-6

    pair = torch.stack([fwd, -fwd], 1).contiguous()
    zero = fwd.clone()
    zero[9] = 0.0
    edges = torch.tensor([F32(np.pi), np.nextafter(F32(-np.pi), F32(0)), F32(0)], dtype=torch.float32).repeat(B, 1)
    Kd = K.cuda()
    _, (b1, b2, b3, keep), params2 = ops.augment_clouds(x, SEED, STREAM, [pair.cuda(), zero.cuda(), edges.cuda(), Kd],
                                                        ["axis", "dir8", "angle", "keep"], dirs8=DIRS_8.cuda())
    assert _same(_np(params2), _np(params)) and keep is Kd
    assert _same(_np(b1), ar.axes(pair.numpy(), c, s))
    assert _same(_np(b2), ar.dir8(zero.numpy(), c, s, DIRS_8.numpy()))
    assert _same(_np(b2)[9], np.full(8, 0.125, F32)) and np.abs(_np(b2).astype(np.float64).sum(1) - 1).max() <= 2e-7
    assert _same(_np(b3), ar.shift_angles(edges.numpy(), th))
    e = _np(b3).astype(np.float64)
    assert (e > -np.pi - 2e-7).all() and (e <= np.pi + 2e-7).all()
    assert ar.angular_distance(e, edges.numpy().astype(np.float64) - th[:, None]).max() <= 1e-6


def test_jitter_values_and_moments(ops):
    B, N, sigma = 64, 1024, 0.01
    clip = 5 * sigma
    z = torch.zeros(B, N, 3).cuda()
    out, _, params = ops.augment_clouds(z, SEED, STREAM, jitter=(sigma, clip))
    got = _np(out).astype(np.float64)
    ref = ar.jitter(SEED, STREAM, B, N, sigma, clip).astype(np.float64)
    assert (np.abs(got) <= float(F32(clip))).all()
    assert (np.abs(got - ref) <= 2.0 ** -22 * np.abs(ref)).all()
    n = got.size
    print("jitter mean", got.mean(), "std", got.std(), "sigma", sigma)
    assert abs(got.mean()) <= 5 * sigma / math.sqrt(n)
    assert abs(got.std() - sigma) <= 5 * sigma / math.sqrt(2 * n)

    x = torch.randn(4, 300, 3, generator=torch.Generator().manual_seed(3))
    out, _, params = ops.augment_clouds(x.cuda(), SEED, STREAM, jitter=(sigma, sigma))
    _, c, s, sc = _check_params(params, 4)
    rot = ar.points(x.numpy(), c, s, sc).astype(np.float64)
    j = ar.jitter(SEED, STREAM, 4, 300, sigma, sigma).astype(np.float64)
    assert (np.abs(j) <= float(F32(sigma))).all() and (np.abs(j) == float(F32(sigma))).any()
    assert (np.abs(_np(out).astype(np.float64) - (rot + j)) <= 2.0 ** -22 * (np.abs(rot) + np.abs(j))).all()


def test_scale_after_rotation(ops):
    x = torch.randn(16, 40, 6, generator=torch.Generator().manual_seed(4))
    out, _, params = ops.augment_clouds(x.cuda(), SEED, STREAM, scale=(0.8, 1.25))
    _, c, s, sc = _check_params(params, 16, scale=(0.8, 1.25))
    assert (sc >= F32(0.8)).all() and (sc < F32(1.25)).all() and len(set(sc.tolist())) == 16
    assert _same(_np(out), ar.points(x.numpy(), c, s, sc, use_scale=True))       # fl(fl(rotation) * scale); normals not scaled


def test_determinism_and_streams(ops):
    import dataloader_common as dc
    from pnpp_hip.augment import Augment
    x = torch.randn(3, 50, 3, generator=torch.Generator().manual_seed(5)).cuda()
    mu = torch.zeros(3).cuda()
    run = lambda stream: ops.augment_clouds(x, SEED, stream, [mu], ["angle"], jitter=(0.01, 0.05), scale=(0.9, 1.1))
    a, b, other = run(STREAM), run(STREAM), run(STREAM + 1)
    assert _same(_np(a[0]), _np(b[0])) and _same(_np(a[1][0]), _np(b[1][0])) and _same(_np(a[2]), _np(b[2]))
    assert not _same(_np(a[0]), _np(other[0])) and not _same(_np(a[2]), _np(other[2]))
    aug = Augment(seed=SEED, scale=(0.9, 1.1), jitter=(0.01, 0.05))
    bank = dc.DeviceCloudBank([_np(x[i]) for i in range(3)], "cuda", seed=SEED)
    bank.sample([0, 1, 2], 16)
    got = aug(x, mu, kinds=("angle",))
    assert aug.draws == bank.draws == 1 and _same(_np(got[0]), _np(a[0])) and _same(_np(aug.last_params), _np(a[2]))
    assert not _same(_np(run(bank.draws)[2]), _np(aug.last_params))             # the bank's stream of that number: other words


def test_bank_loader_batches_are_the_plain_ones_transformed(ops, gt):
    import dataloader_common as dc
    from pnpp_hip.augment import Augment
    rng = np.random.default_rng(6)
    clouds = [rng.standard_normal((40 + 3 * i, 3)).astype(np.float32) for i in range(6)]
    mu = gt["mu"][:6]

    def loader(**kw):
        return dc.BankLoader(dc.DeviceCloudBank(clouds, "cuda", seed=11), [mu], 32, 4, True, seed=12, **kw)

    aug = Augment(seed=SEED)
    it = iter(loader(augment=aug, kinds=("angle",)))
    order = torch.randperm(6, generator=torch.Generator().manual_seed(12))
    for i, (px, pmu) in enumerate(loader()):
        ax, amu = next(it)
        p = _np(aug.last_params)
        Bn = px.shape[0]
        assert _same(_np(pmu), mu.numpy()[order[4 * i:4 * i + 4].numpy()])
        assert _same(_np(ax), ar.points(_np(px), p[:, 0], p[:, 1], p[:, 2]))
        th = ar.theta(SEED, ar.STREAM_BASE | (i + 1), Bn)
        assert _same(p[:, 3], th.astype(F32)) and _same(_np(amu), ar.shift_angles(_np(pmu), th))
    assert aug.draws == 2 and next(it, None) is None


def test_all_switches_off_is_a_copy(ops, gt):
    x = torch.randn(4, 257, 6, generator=torch.Generator().manual_seed(7))
    x[0, 0, 0], x[1, 5, 2] = -0.0, float("inf")
    mu, fwd, vm3, K = gt["mu"][:4], gt["fwd"][:4], gt["vm3"][:4], gt["K"][:4]
    out, (a, f, v), params = ops.augment_clouds(x.cuda(), SEED, STREAM, [mu.cuda(), fwd.cuda(), vm3.cuda()], ["angle", "axis", "vm"],
                                                counts=K.cuda(), yaw=False)
    assert _same(_np(out), x.numpy()) and _same(_np(a), mu.numpy()) and _same(_np(f), fwd.numpy()) and _same(_np(v), vm3.numpy())
    assert _same(_np(params), np.tile(np.array([1, 0, 1, 0], F32), (4, 1)))


@pytest.mark.parametrize("name,ckpt", [("train_single_peak_vonMises_KL", "vonMises_best.pth"),
                                       ("train_multi_peaks_vonMises_KL", "mvM_best.pth"), ("train_8dir_KL", "8dir_KLdiv_0926.pth")])
def test_scripts_train_with_augment(name, ckpt, tmp_path, monkeypatch):
    """--augment --synthetic through the scripts' own loop: the train split goes through AugmentedLoader (for the 8-direction
    script the labels come out of the launch), the step is still captured, the losses are finite numbers."""
    import importlib
    from pnpp_hip import trainer
    mod = importlib.import_module(name)
    monkeypatch.setattr(mod, "RES", tmp_path)
    monkeypatch.setattr(mod, "FIGS", tmp_path / "figs")
    monkeypatch.setattr(mod, "EPOCHS", 2)
    monkeypatch.setattr(mod, "BATCH", 16)
    monkeypatch.setattr(mod, "NUM_POINTS", 256)
    seen = []
    real = trainer.AugmentedLoader.__iter__

    def spy(self):
        for batch in real(self):
            seen.append((self.augment.draws, self.augment.last_params[:, 3].clone()))
            yield batch

    monkeypatch.setattr(trainer.AugmentedLoader, "__iter__", spy)
    hist, test_loss = mod.main(["--synthetic", "64", "--sampler", "device", "--augment"])
    train = hist["total"]["train"] if "total" in hist else hist["train"]
    assert len(train) == 2 and all(v == v and 0 < v < 20.0 for v in train) and test_loss == test_loss
    assert (tmp_path / ckpt).exists()
    steps = hist["_trainer"]["steps"] if "_trainer" in hist else hist["steps"]
    assert steps["graph"] >= 1                                                     # the loader runs outside the captured step
    assert [d for d, _ in seen] == list(range(1, 7))                               # 44 train clouds: 3 batches x 2 epochs, all augmented
    assert not torch.equal(seen[0][1], seen[3][1])                                 # the same position, next epoch: another pose
