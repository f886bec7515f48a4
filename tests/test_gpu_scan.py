"""GPU parity of the raw-scan preparation (csrc/scan_kernels.hip) against its CPU restatement (tests/scan_ref.py).

Bar: rows, lengths' and index bit-equal -- the zero padding included -- to the restatement.  The voxel step is integers, float32
operations in a fixed order and order-free minima; the outlier statistic is held bit-equal to the restatement fed the device's own
neighbour lists, mean / std / thr to 1e-12 relative of numpy's float64 (the summation orders differ), and the keep mask on every row
(no row lies within 1e-6 thr of the threshold, which the tests assert on the restatement first); the unit frame's centroid lies within
one float32 spacing of numpy's (again the summation order) and, given the device's centre, every row is bit-equal."""
import numpy as np
import pytest
import torch

import scan_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]        # wave, tile and running-base edges
GRIDS = [1, 2, 32, 1024]
SHAPES = [(3, 1), (6, 1), (3, 3), (6, 3)]                 # (C, B)


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


def _cloud(rng, B, N, C):
    x = rng.standard_normal((B, N, C)).astype(F32)
    x[..., :3] = (x[..., :3] * np.array([1.0, 0.6, 0.3]) + np.array([3.0, -20.0, 0.25])).astype(F32)   # off centre, uneven extents
    return x


def _ragged(x, lengths):
    for b, n in enumerate(lengths):
        x[b, n:] = np.nan
    return x


def _check_voxel(ops, x, lengths=None, **kw):
    x = np.ascontiguousarray(x, F32)
    xd = torch.from_numpy(x).cuda()
    out, kept, idx = ops.voxel_downsample(xd, lengths=_dev_lengths(lengths), index=True, **kw)
    assert out.shape == x.shape and out.data_ptr() != xd.data_ptr() and kept.dtype == idx.dtype == torch.int32
    out2, kept2 = ops.voxel_downsample(xd, lengths=_dev_lengths(lengths), **kw)
    assert torch.equal(kept, kept2) and _same(_np(out), _np(out2))               # two calls, the same bits
    out, kept, idx = _np(out), _np(kept), _np(idx)
    ref = R.voxel_downsample(x, lengths=lengths, **kw)
    assert _same(kept, ref[1]), (kept, ref[1])
    assert _same(idx, ref[2])
    assert _same(out, ref[0])
    assert _same(_np(xd), x)                                                   # out of place
    return out, kept, idx


@pytest.mark.parametrize("N", SIZES)
def test_voxel_size_grid_bit_equal(ops, N):
    """Every grid and a clamping cell at this N, the four (C, B) shapes in turn; B = 3 alternates uniform and ragged (lengths 1, N
    and one between, NaN in the padding)."""
    rng = np.random.default_rng(N)
    turn = SIZES.index(N)
    for gi, kw in enumerate([{"grid": g} for g in GRIDS] + [{"cell": 1e-4}]):
        C, B = SHAPES[(turn + gi) % 4]
        x = _cloud(rng, B, N, C)
        lengths = None
        if B == 3 and (gi + turn) % 2:
            lengths = [1, N, max(1, (2 * N) // 3)]
            _ragged(x, lengths)
        out, kept, idx = _check_voxel(ops, x, lengths, **kw)
        assert (kept >= 1).all() and not np.isnan(out).any()
        if kw.get("grid") == 1:
            assert (kept == 1).all()
        if "cell" in kw and N > 2:                                             # extents of several units over 1e-4: the clamp is hit
            q = np.floor((x[0, :, :3] - x[0, :, :3].min(0)) / F32(kw["cell"]))
            assert lengths is not None or (q > R.MAX_CELL).any()


def test_voxel_many_clouds_one_launch(ops):
    x = _cloud(np.random.default_rng(65), 65, 300, 3)
    lengths = [1 + (37 * b) % 300 for b in range(65)]
    _check_voxel(ops, _ragged(x, lengths), lengths, grid=8)
    _check_voxel(ops, _cloud(np.random.default_rng(66), 65, 130, 6), None, cell=0.5)


def test_voxel_every_row_its_own_cell_and_identical_rows(ops):
    g = np.arange(16, dtype=F32)
    lat = np.stack(np.meshgrid(g, g, g[:8], indexing="ij"), -1).reshape(1, 2048, 3)
    lat = lat[:, np.random.default_rng(0).permutation(2048)]
    out, kept, idx = _check_voxel(ops, lat, cell=1.0)                            # 2,048 occupied cells in 4,096 slots: load 0.5, the fullest
    assert kept[0] == 2048 and _same(out, lat) and np.array_equal(idx[0], np.arange(2048))
    out, kept, idx = _check_voxel(ops, np.concatenate([lat, lat[:, ::-1]]), grid=16)   # the same through grid=: h = 15 / 16
    assert (kept <= 2048).all() and (kept >= 1024).all()
    same = np.tile(np.array([0.3, -1.5, 2.0], F32), (2, 1500, 1))
    for kw in ({"grid": 32}, {"cell": 0.01}):
        out, kept, idx = _check_voxel(ops, same, **kw)                           # extent 0: h = 1 (grid), one cell either way
        assert (kept == 1).all() and (idx[:, 0] == 0).all() and (idx[:, 1:] == -1).all()


def test_voxel_integer_lattice_equal_keys_lowest_row_wins(ops):
    """Cells of edge 3 over integer coordinates 0..8: a cell holds 0, 1, 2 per axis, its centre is 1.5, so rows at 1 and 2 are equally
    near on every axis -- eight rows with the same d per cell, and the lowest row has to win."""
    g = np.arange(9, dtype=F32)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(729, 3)
    x = np.stack([lat, lat[::-1], lat[np.random.default_rng(3).permutation(729)]])
    _, ids, d, _ = R.voxel_cells(x[2], cell=3.0)
    ties = sum(int((d[ids == c] == d[ids == c].min()).sum() == 8) for c in np.unique(ids))
    assert ties == 27                                                          # the restatement sees the ties the test is about
    out, kept, idx = _check_voxel(ops, x, cell=3.0)
    assert (kept == 27).all()
    x6 = np.concatenate([x, np.arange(3 * 729 * 3, dtype=F32).reshape(3, 729, 3)], -1)
    out, kept, idx = _check_voxel(ops, x6, cell=3.0)                             # columns 3..5 ride along with their rows
    assert _same(out[1, :27, 3:], x6[1, idx[1, :27], 3:])


# ---- outliers -------------------------------------------------------------------------------------------------------------
def _check_outliers(ops, x, k, std_ratio, lengths=None):
    """The device against the restatement fed the device's own lists; -> (kept, stats) as numpy."""
    x = np.ascontiguousarray(x, F32)
    B, N, C = x.shape
    xd, ld = torch.from_numpy(x).cuda(), _dev_lengths(lengths)
    out, kept, idx, stats = ops.remove_outliers(xd, k, std_ratio, lengths=ld, index=True, stats=True)
    again = ops.remove_outliers(xd, k, std_ratio, lengths=ld, index=True, stats=True)
    assert all(_same(_np(a), _np(b)) for a, b in zip((out, kept, idx, stats), again))   # two calls, the same bits
    pts = xd[..., :3].contiguous()
    lists = ops.knn(pts, pts, min(k + 1, N), ld)
    if lists.shape[2] < k + 1:
        lists = lists.new_zeros(B, N, k + 1)
    stat = _np(ops.outlier_statistic(xd, lists, ld))
    out, kept, idx, stats = _np(out), _np(kept), _np(idx), _np(stats)
    ref = R.remove_outliers(x, k, std_ratio, lengths, lists=_np(lists))
    for b in range(B):
        Nv = R.valid_rows(lengths, b, N)
        assert _same(stat[b, :Nv], ref[4][b, :Nv]) and (stat[b, Nv:] == 0).all()   # the per-point statistic, bit for bit
        if Nv > k:
            thr = ref[3][b, 2]
            assert np.abs(ref[4][b, :Nv] - thr).min() >= 1e-6 * thr              # no row near the threshold: none is left out below
            np.testing.assert_allclose(stats[b, :3], ref[3][b, :3], rtol=1e-12, atol=0)
        else:
            assert _same(stats[b], ref[3][b])                                   # passed through whole: [0, 0, inf, Nv]
    assert _same(kept, ref[1]), (kept, ref[1])
    assert _same(idx, ref[2])
    assert _same(out, ref[0])
    assert _same(stats[:, 3], ref[1].astype(np.float64))
    assert _same(_np(xd), x)
    return kept, stats


def _contaminated_batch(N, seeds, C=3):
    xs, inj = zip(*(R.contaminated(("sphere", "box")[i % 2], N, s) for i, s in enumerate(seeds)))
    x = np.stack(xs)
    if C == 6:
        x = np.concatenate([x, np.random.default_rng(N).standard_normal(x.shape).astype(F32)], -1)
    return x, np.stack(inj)


@pytest.mark.parametrize("k,std_ratio,N,C", [(1, 1.0, 1025, 3), (3, 2.0, 2049, 6), (16, 2.0, 1024, 3), (127, 1.0, 1024, 6)])
def test_outliers_bit_equal(ops, k, std_ratio, N, C):
    x, inj = _contaminated_batch(N, (0, 1, 2), C)
    kept, stats = _check_outliers(ops, x, k, std_ratio)
    assert (kept < N).all() and (kept > 0.9 * N).all()


def test_outliers_own_lists_agree(ops):
    """The restatement on its own brute-force lists keeps the same rows as the device on the search's."""
    x, inj = _contaminated_batch(1024, (0, 1))
    out, kept, idx = ops.remove_outliers(torch.from_numpy(x).cuda(), 8, 1.0, index=True)
    ref = R.remove_outliers(x, 8, 1.0)
    assert np.abs(ref[4] - ref[3][:, 2:3]).min() >= 1e-6 * ref[3][:, 2].max()
    assert _same(_np(kept), ref[1]) and _same(_np(idx), ref[2]) and _same(_np(out), ref[0])
    for b in range(2):
        rows = idx.cpu().numpy()[b, : ref[1][b]]
        assert inj[b][rows].mean() < 0.02 and (~inj[b]).sum() == (~inj[b][rows]).sum()   # nearly all injected rows gone, no surface row


def test_outliers_ragged_short_clouds_pass_through(ops):
    x, _ = _contaminated_batch(300, (0, 1, 2, 3, 4))
    lengths = [300, 16, 17, 1, 200]                                            # k = 16: 16 and 1 pass through, 17 is filtered
    kept, stats = _check_outliers(ops, _ragged(x, lengths), 16, 2.0, lengths)
    assert kept[1] == 16 and kept[3] == 1 and np.isinf(stats[1, 2]) and kept[2] <= 17
    x, _ = _contaminated_batch(12, (5, 6))
    kept, stats = _check_outliers(ops, _ragged(x, [12, 5]), 16, 2.0, [12, 5])     # padded to fewer than k + 1 rows: all pass through
    assert kept.tolist() == [12, 5]
    with pytest.raises(ValueError, match="neighbours"):
        ops.remove_outliers(torch.from_numpy(x).cuda(), 16, 2.0)
    x65 = _cloud(np.random.default_rng(7), 65, 40, 6)
    lengths = [1 + (7 * b) % 40 for b in range(65)]
    _check_outliers(ops, _ragged(x65, lengths), 3, 1.5, lengths)


# ---- unit frame -----------------------------------------------------------------------------------------------------------
def _check_normalize(ops, x, lengths=None, **kw):
    x = np.ascontiguousarray(x, F32)
    xd = torch.from_numpy(x).cuda()
    out, c, r = ops.normalize_clouds(xd, lengths=_dev_lengths(lengths), **kw)
    out2, c2, r2 = ops.normalize_clouds(xd, lengths=_dev_lengths(lengths), **kw)
    assert _same(_np(out), _np(out2)) and _same(_np(c), _np(c2)) and _same(_np(r), _np(r2))
    out, c, r = _np(out), _np(c), _np(r)
    own = R.normalize_clouds(x, lengths, kw.get("centre", "centroid"), kw.get("scale", "sphere"))
    assert (np.abs(c.astype(np.float64) - own[1]) <= np.spacing(np.abs(own[1]))).all()   # one float32 spacing: the summation order
    if kw.get("centre", "centroid") != "centroid":
        assert _same(c, own[1])
    ref = R.normalize_clouds(x, lengths, kw.get("centre", "centroid"), kw.get("scale", "sphere"), given_centre=c)
    assert _same(r, ref[2]), (r, ref[2])
    assert _same(out, ref[0])
    assert _same(_np(xd), x)
    return out, c, r


@pytest.mark.parametrize("N", SIZES)
def test_normalize_size_grid_bit_equal(ops, N):
    rng = np.random.default_rng(100 + N)
    turn = SIZES.index(N)
    modes = [(c, s) for c in ("centroid", "box", None) for s in ("sphere", "box", None)]
    for mi, (centre, scale) in enumerate(modes):
        C, B = SHAPES[(turn + mi) % 4]
        x = _cloud(rng, B, N, C)
        lengths = None
        if B == 3 and (mi + turn) % 2:
            lengths = [1, N, max(1, (2 * N) // 3)]
            _ragged(x, lengths)
        out, c, r = _check_normalize(ops, x, lengths, centre=centre, scale=scale)
        assert not np.isnan(out).any() and (r > 0).all()
        if scale == "sphere":
            for b in range(B):
                Nv = R.valid_rows(lengths, b, N)
                n = np.linalg.norm(out[b, :Nv, :3].astype(np.float64), axis=1).max()
                assert n == 0.0 or abs(n - 1.0) < 1e-6


def test_normalize_many_clouds_and_identical_rows(ops):
    x = _cloud(np.random.default_rng(65), 65, 300, 6)
    lengths = [1 + (37 * b) % 300 for b in range(65)]
    _check_normalize(ops, _ragged(x, lengths), lengths)
    same = np.tile(np.array([0.3, -1.5, 2.0], F32), (2, 100, 1))
    out, c, r = _check_normalize(ops, same, centre="box", scale="box")
    assert (r == 1).all() and (out == 0).all()


# ---- the chain ------------------------------------------------------------------------------------------------------------
def _scan(rng, B, N):
    """raw scans: a contaminated surface, denser on one half, anywhere and of any size"""
    xs = []
    for b in range(B):
        p, _ = R.contaminated(("sphere", "box")[b % 2], N, int(rng.integers(1 << 30)))
        xs.append(p * F32(rng.uniform(0.5, 2.0)) + rng.uniform(-5, 5, 3).astype(F32))
    return np.stack(xs)


def test_scan_prep_end_to_end(ops):
    from pnpp_hip.scans import STREAM_BASE, ScanPrep
    x = _scan(np.random.default_rng(11), 4, 3000)
    xd = torch.from_numpy(x).cuda()
    prep = ScanPrep(grid=32, outlier_k=8, outlier_std=1.0, resample=1024, seed=5)
    out, lengths, frame = prep(xd)
    assert out.shape == (4, 1024, 3) and (lengths == 1024).all() and frame.centre.shape == (4, 3) and frame.scale.shape == (4,)
    v = R.voxel_downsample(x, grid=32)
    o = R.remove_outliers(v[0], 8, 1.0, v[1])
    assert np.abs(o[4] - o[3][:, 2:3])[o[4] > 0].min() >= 1e-6 * o[3][:, 2].max()
    assert _same(_np(prep.last_lengths), o[1])
    n = R.normalize_clouds(o[0], o[1], given_centre=_np(frame.centre))
    assert _same(_np(frame.scale), n[2])
    want = ops.subsample_points(5, STREAM_BASE | 1, torch.from_numpy(n[0]).cuda(), torch.from_numpy(o[1]).cuda(), 1024)
    assert _same(_np(out), _np(want))                                           # the chain is its steps, the draw is 2^60 | 1
    norms = np.linalg.norm(_np(out).astype(np.float64), axis=-1)
    assert norms.max() <= 1.0 + 1e-6 and np.abs(_np(out).mean(1)).max() < 0.2      # a unit frame came out
    again = ScanPrep(grid=32, outlier_k=8, outlier_std=1.0, resample=1024, seed=5)(xd)
    assert _same(_np(again[0]), _np(out)) and _same(_np(again[2].centre), _np(frame.centre))
    ragged = ScanPrep(cell=0.25, outlier_k=None, centre="box", scale="box")(xd)
    assert ragged[0].shape == x.shape and (ragged[1] < 3000).all() and prep.draws == 1


def test_three_steps_replay_in_a_graph(ops):
    x = torch.from_numpy(_scan(np.random.default_rng(12), 3, 1500)).cuda()

    def steps():
        a, la = ops.voxel_downsample(x, grid=16)
        b, lb, st = ops.remove_outliers(a, 8, 1.0, la, stats=True)
        c, centre, scale = ops.normalize_clouds(b, lb)
        return c, lb, st, centre, scale

    eager = [t.clone() for t in steps()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        steps()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = steps()
    for t in captured:
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same(_np(a), _np(b)) for a, b in zip(eager, captured))


def test_bank_loader_prepare(ops):
    from dataloader_common import BankLoader, DeviceCloudBank
    from pnpp_hip.scans import ScanPrep
    rng = np.random.default_rng(13)
    clouds = [_scan(rng, 1, n)[0] for n in (2500, 1800, 3000)]
    bank = DeviceCloudBank(clouds, "cuda", seed=3)
    target = torch.arange(3, dtype=torch.float32)
    loader = BankLoader(bank, [target], 512, 3, shuffle=False, prepare=ScanPrep(grid=24, outlier_k=8, outlier_std=1.0, resample=512))
    (xyz, t), = list(loader)
    assert xyz.shape == (3, 512, 3) and torch.equal(t.cpu(), target) and bank.draws == 0
    assert np.linalg.norm(_np(xyz).astype(np.float64), axis=-1).max() <= 1.0 + 1e-6
    from pnpp_hip import trainer
    raw = torch.from_numpy(_scan(rng, 6, 700))
    loaders = trainer.prepared({"train": trainer.SyntheticLoader([raw, torch.arange(6.0)], 4, False, torch.device("cuda"))}, 256, 0)
    batches = list(loaders["train"])                                            # what --prepare puts around every split's loader
    assert [tuple(b[0].shape) for b in batches] == [(4, 256, 3), (2, 256, 3)] and torch.equal(batches[1][1].cpu(), torch.tensor([4.0, 5.0]))
    assert np.linalg.norm(_np(batches[0][0]).astype(np.float64), axis=-1).max() <= 1.0 + 1e-6
    with pytest.raises(ValueError, match="prepare.resample"):
        BankLoader(bank, [target], 512, 3, shuffle=False, prepare=ScanPrep(grid=24, resample=256))
