"""Yaw symmetry on the device against the float32 restatement (tests/symmetry_ref.py).

Gates: nearest_dist and nearest_idx bit-equal; distance and floor within one float32 spacing, |a - b| <= 2^-23 |b| -- a float64 sum of at
most 2^20 float32 terms is order-independent to ~1e-10, so after the one rounding the two sides are equal or adjacent; the decision equal
to the restatement's decision applied to the device's own D and nu."""
import math

import numpy as np
import pytest
import torch

import symmetry_ref as R

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    """Equal bit for bit (a NaN score of a one-point cloud included)."""
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want)))


def _check_decision(sym, G, orders=R.ORDERS, tol=R.TOL):
    """order, count, angles and score against the restatement's decision on the device's own D and nu."""
    D, nu = sym.profile.distance.cpu().numpy(), sym.profile.floor.cpu().numpy()
    for b in range(D.shape[0]):
        order, count, angles = R.decide(D[b], nu[b], tol, orders)
        assert int(sym.order[b]) == order and int(sym.count[b]) == count, (b, order, int(sym.order[b]))
        assert np.array_equal(sym.angles[b].cpu().numpy(), angles)
        with np.errstate(divide="ignore", invalid="ignore"):
            score = R.symmetric(D[b]) / (np.float32(2.0) * nu[b])
        assert np.array_equal(sym.score[b].cpu().numpy(), score, equal_nan=True)


def _check_parity(x, centre, G=None, angles=None, lengths=None):
    """x (B, N, 3) numpy, centre "centroid" or (B, 3) numpy.  The profile call with nearest=True against the restatement, cloud by cloud;
    on the uniform grid also the symmetry call: the same profile bit for bit, and its decision."""
    from pnpp_hip import symmetry
    B, N = x.shape[:2]
    c = "centroid" if isinstance(centre, str) else _dev(centre)
    kw = dict(centre=c, lengths=lengths)
    prof = symmetry.yaw_profile(_dev(x), num=G, nearest=True, **kw) if angles is None else \
        symmetry.yaw_profile(_dev(x), angles=_dev(angles), nearest=True, **kw)
    table = prof.table.cpu().numpy()
    if angles is None:
        assert np.array_equal(table, R.grid_table(G))
    else:
        assert table.shape == (len(angles), 2)
    for b in range(B):
        nv = N if lengths is None else int(lengths[b])
        cb = R.centroid(x[b, :nv]) if isinstance(centre, str) else centre[b]
        D, nu, nd, ni = R.profile(x[b, :nv], cb, table, nearest=True)
        assert np.array_equal(prof.nearest_dist[b, :, :nv].cpu().numpy(), nd), b
        assert np.array_equal(prof.nearest_idx[b, :, :nv].cpu().numpy(), ni), b
        assert torch.all(prof.nearest_dist[b, :, nv:] == 0) and torch.all(prof.nearest_idx[b, :, nv:] == -1)
        assert _close(prof.distance[b].cpu().numpy(), D), (b, prof.distance[b].cpu().numpy(), D)
        assert _close(float(prof.floor[b]), nu), (b, float(prof.floor[b]), nu)
    plain = symmetry.yaw_profile(_dev(x), num=G, **kw) if angles is None else symmetry.yaw_profile(_dev(x), angles=_dev(angles), **kw)
    assert plain.nearest_dist is None and torch.equal(plain.distance, prof.distance) and torch.equal(plain.floor, prof.floor)
    if angles is None:
        sym = symmetry.yaw_symmetry(_dev(x), num=G, **kw)
        assert torch.equal(sym.profile.distance, prof.distance) and torch.equal(sym.profile.floor, prof.floor)
        assert sym.angles.shape == (B, max(R.ORDERS))
        _check_decision(sym, G)
    return prof


@pytest.mark.parametrize("B", R.PARITY_B)
@pytest.mark.parametrize("N", R.PARITY_N)
def test_parity_small(N, B):
    x = R.parity_cloud(B, N)
    for G in R.PARITY_G:
        prof = _check_parity(x, "centroid", G)
        assert torch.all(prof.distance[:, 0] == 0)


@pytest.mark.parametrize("N", R.TILE_N)
def test_parity_across_tiles(N):
    from pnpp_hip import _lib
    assert _lib.YAW_TILE == R.TILE and _lib.YAW_ANGLE_BLOCK == R.ANGLE_BLOCK
    _check_parity(R.parity_cloud(1, N, seed=N % 5), "centroid", 3)


def test_parity_lattice_ties():
    x, c = R.lattice()
    for G in (4, 72):
        prof = _check_parity(x[None], c[None], G)
        assert torch.all(prof.distance[0, [0, G // 4, G // 2, 3 * G // 4]] == 0) and float(prof.floor[0]) == 1.0
    two = np.stack([x, x[::-1]])                                      # a second order of the same points: other ties, other winners
    _check_parity(two, np.stack([c, c]), 8)


def test_parity_angles_tensor():
    angles = np.array([0.0, 0.3, 1.0, 2.5, math.pi, 4.0, 5.5, 6.0, 7.0, -1.0, 0.3], np.float32)
    _check_parity(R.parity_cloud(2, 100, seed=3), "centroid", angles=angles)
    _check_parity(R.parity_cloud(2, 100, seed=3), np.zeros((2, 3), np.float32), angles=angles[:1])


def test_parity_many_clouds():
    _check_parity(R.parity_cloud(65, 64, seed=1), "centroid", 9)


def test_one_point_cloud():
    from pnpp_hip import symmetry
    sym = symmetry.yaw_symmetry(_dev(np.array([[[0.25, -1.5, 3.0]]], np.float32)), num=8)
    assert float(sym.profile.floor[0]) == 0.0 and torch.all(sym.profile.distance == 0) and int(sym.order[0]) == 0


def test_ragged():
    """Lengths 1, 2, mid, N and NaN in the padding: every row bit-equal to the uniform call on that cloud alone; nearest 0 / -1 there."""
    from pnpp_hip import symmetry
    for N, G in ((300, 9), (R.TILE + 40, 3)):
        lens = [1, 2, N // 2 + 1, N]
        x = R.parity_cloud(4, N, seed=2)
        for b, n in enumerate(lens):
            x[b, n:] = np.nan
        xd = _dev(x)
        both = lambda x, **kw: (symmetry.yaw_profile(x, num=G, nearest=True, **kw), symmetry.yaw_symmetry(x, num=G, **kw))
        prof, sym = both(xd, lengths=lens)
        on_device = both(xd, lengths=torch.tensor(lens, dtype=torch.int32).cuda())
        for b, n in enumerate(lens):
            p1, s1 = both(xd[b:b + 1, :n].contiguous())
            for p, s in ((prof, sym), on_device):
                for got in (p, s.profile):
                    assert torch.equal(got.distance[b:b + 1], p1.distance) and torch.equal(got.floor[b:b + 1], p1.floor)
                assert torch.equal(p.nearest_dist[b:b + 1, :, :n], p1.nearest_dist)
                assert torch.equal(p.nearest_idx[b:b + 1, :, :n], p1.nearest_idx)
                assert torch.all(p.nearest_dist[b, :, n:] == 0) and torch.all(p.nearest_idx[b, :, n:] == -1)
                assert torch.equal(s.order[b:b + 1], s1.order) and torch.equal(s.angles[b:b + 1], s1.angles)
                assert _same_bits(s.score[b:b + 1], s1.score)
        _check_decision(sym, G)
    _check_parity(x[:, :300].copy(), "centroid", 7, lengths=[1, 2, 151, 300])


@pytest.fixture(scope="module")
def class_clouds():
    """The fifteen classification cases (tests/test_symmetry_cpu.py holds that the float64 restatement admits every one of them)."""
    names = [n for n in R.FAMILIES for _ in R.CLASS_SEEDS]
    x = np.stack([R.family(n, R.CLASS_N, s) for n in R.FAMILIES for s in R.CLASS_SEEDS])
    return x, [R.FAMILIES[n] for n in names]


def test_classification(class_clouds):
    from pnpp_hip import symmetry
    x, want = class_clouds
    sym = symmetry.yaw_symmetry(_dev(x), num=R.CLASS_G, tol=R.TOL)
    assert sym.order.tolist() == want and sym.count.tolist() == want
    _check_decision(sym, R.CLASS_G)
    rng = np.random.default_rng(R.SEED)
    again = np.stack([R.turned(c, t) for c, t in zip(x, rng.uniform(0, 2 * math.pi, len(x)))])
    assert symmetry.yaw_symmetry(_dev(again), num=R.CLASS_G, tol=R.TOL).order.tolist() == want
    sym72 = symmetry.yaw_symmetry(_dev(x))                            # the defaults: 72 angles
    assert sym72.order.tolist() == want


def test_deterministic_and_capturable():
    from pnpp_hip import symmetry
    x = _dev(R.parity_cloud(3, 700, seed=4))
    def call():
        sym, prof = symmetry.yaw_symmetry(x, num=24), symmetry.yaw_profile(x, num=24, nearest=True)
        return (sym.order, sym.count, sym.angles, sym.score, sym.profile.distance, sym.profile.floor, *prof)
    for s, t in zip(call(), call()):
        assert _same_bits(s, t)
    static = x.clone()
    lens = torch.tensor([700, 650, 3], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = symmetry.yaw_symmetry(static, num=24, lengths=lens)
    fresh = _dev(R.parity_cloud(3, 700, seed=1))
    static.copy_(fresh)
    lens.copy_(torch.tensor([5, 700, 699], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    eager = symmetry.yaw_symmetry(fresh, num=24, lengths=lens)
    assert torch.equal(out.profile.distance, eager.profile.distance) and torch.equal(out.profile.floor, eager.profile.floor)
    assert torch.equal(out.order, eager.order) and torch.equal(out.angles, eager.angles) and _same_bits(out.score, eager.score)


def test_bank_symmetry():
    from dataloader_common import DeviceCloudBank
    names = [n for n in R.FAMILIES for _ in range(2)]
    sizes = [1500, 3000, 1777, 2048, 2500, 1501, 2999, 2222, 1900, 2750]
    bank = DeviceCloudBank([R.family(n, size, 40 + i) for i, (n, size) in enumerate(zip(names, sizes))], "cuda")
    sym = bank.symmetry(num_points=1024, chunk=4)
    assert sym.order.shape == (10,) and sym.profile.distance.shape == (10, 72) and sym.score.shape == (10, 72)
    assert sym.order.tolist() == [R.FAMILIES[n] for n in names]
