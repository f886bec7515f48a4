"""Surface normals on the device (pnpp_hip.normals, knn_normals_kernel) against the numpy float64 restatement (tests/normals_ref.py).

The gates come from the number formats, not from what the kernel gives (normals_ref: ANGLE_GATE, NORM_GATE, CURV_GATE): the neighbour
lists are bit-equal to ops.knn, the normal is within 2.5e-7 rad of the restatement fed those lists, of unit norm within 2e-7 and of the
restatement's sign, the curvature within 6e-8.  A point is left out only where the restatement itself reports an ill-conditioned
eigenvector or a sign tie, at most 2 % of a case; those points are still finite and of unit or zero norm."""
import numpy as np
import pytest
import torch

import normals_ref as R

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _orient_args(orient, xyz_dev, lengths=None):
    """orient of the case table -> (what pnpp_hip.normals takes, the restatement's (ref, mode))."""
    from pnpp_hip import normals
    if orient is None:
        return None, (None, "none")
    if orient == "centroid":
        return "centroid", (normals.reference_points(xyz_dev, lengths).cpu().numpy(), "away")
    view = torch.tensor(orient, dtype=torch.float32)
    return view.cuda(), (np.tile(view.numpy(), (xyz_dev.shape[0], 1)), "toward")


def _gates(name, xyz, got_n, got_c, got_idx, ref, mode):
    """Every gate of the module docstring on one uniform batch (numpy arrays); returns the restatement's outputs."""
    n64, c64, ill, tie = R.normals_ref(xyz, got_idx, ref, mode)
    g = got_n.astype(np.float64)
    norm = np.linalg.norm(g, axis=-1)
    assert np.isfinite(got_n).all() and np.isfinite(got_c).all(), name
    assert np.all((np.abs(norm - 1.0) <= R.NORM_GATE) | (norm == 0.0)), name            # the excluded points too
    out = ill | tie
    keep = ~out
    angle = np.linalg.norm(np.cross(g, n64), axis=-1)
    dc = np.abs(got_c.astype(np.float64) - c64)
    print(f"\n[normals {name}] excluded {out.mean():.4f} (ill {ill.mean():.4f}, tie {tie.mean():.4f}); max angle "
          f"{angle[~ill].max():.3e} rad, max |norm - 1| {np.abs(norm[~ill] - 1.0).max():.3e}, max |d curv| {dc[~ill].max():.3e}")
    assert out.mean() <= R.MAX_EXCLUDED, (name, out.mean())
    assert angle[~ill].max() <= R.ANGLE_GATE, name
    assert np.abs(norm[~ill] - 1.0).max() <= R.NORM_GATE, name
    assert dc[~ill].max() <= R.CURV_GATE, name
    assert np.all((g[keep] * n64[keep]).sum(-1) > 0.0), name                              # the sign, wherever it is no tie
    return n64, c64, ill, tie


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_against_restatement(name):
    from pnpp_hip import normals, ops
    c = R.CASES[name]
    xyz = R.batch(c["families"], c["N"], R.SEED)
    x = _dev(xyz)
    orient, (ref, mode) = _orient_args(c["orient"], x)
    n, curv, idx = normals.estimate_normals(x, c["k"], orient, curvature=True, neighbours=True)
    assert n.shape == xyz.shape and curv.shape == xyz.shape[:2] and idx.shape == xyz.shape[:2] + (c["k"],)
    assert n.dtype == torch.float32 and curv.dtype == torch.float32 and idx.dtype == torch.int32 and not n.requires_grad
    assert torch.equal(idx, ops.knn(x, x, c["k"])), "neighbour lists differ from ops.knn"
    _gates(name, xyz, n.cpu().numpy(), curv.cpu().numpy(), idx.cpu().numpy(), ref, mode)
    # the outputs do not depend on which optional arrays are asked for, and two calls give the same bits
    assert torch.equal(normals.estimate_normals(x, c["k"], orient), n)
    again = normals.estimate_normals(x, c["k"], orient, curvature=True)
    assert torch.equal(again[0], n) and torch.equal(again[1], curv)
    # the six-column layout: the points bit for bit, then the same normals
    six = normals.with_normals(x, c["k"], orient)
    assert six.shape == xyz.shape[:2] + (6,) and torch.equal(six[:, :, :3], x) and torch.equal(six[:, :, 3:], n)


def test_exact_plane_with_viewpoint():
    """z = 0.25 exactly: every normal is +z toward a viewpoint above the plane, every curvature one rounding from 0."""
    from pnpp_hip import normals
    xyz = R.batch(("plane",), 200, R.SEED)
    x = _dev(xyz)
    view = torch.tensor([0.0, 0.0, 5.0]).cuda()
    n, curv, idx = normals.estimate_normals(x, 16, view, curvature=True, neighbours=True)
    _gates("plane", xyz, n.cpu().numpy(), curv.cpu().numpy(), idx.cpu().numpy(), np.array([[0.0, 0.0, 5.0]], np.float32), "toward")
    g = n.cpu().numpy().astype(np.float64)
    assert np.linalg.norm(np.cross(g, np.array([0.0, 0.0, 1.0])), axis=-1).max() <= R.ANGLE_GATE and np.all(g[..., 2] > 0.0)
    assert curv.abs().max().item() <= R.CURV_GATE
    below = normals.estimate_normals(x, 16, torch.tensor([0.0, 0.0, -5.0]).cuda())
    assert np.all(below.cpu().numpy()[..., 2] < 0.0)


def test_sphere_centroid_points_outward():
    from pnpp_hip import normals
    xyz = R.batch(("sphere",), 1024, R.SEED + 7)
    x = _dev(xyz)
    n = normals.estimate_normals(x, 16, "centroid")
    c = normals.reference_points(x)
    assert c.shape == (1, 3) and c.dtype == torch.float32
    assert np.abs(c.cpu().numpy().astype(np.float64) - xyz.astype(np.float64).mean(1)).max() <= 1e-7
    s = (n.double() * (x.double() - c.double()[:, None, :])).sum(-1)
    assert bool((s > 0).all())
    # 1 % radial noise on a shell sampled this densely: the normal is the radial direction to within a few degrees
    radial = torch.nn.functional.normalize(x.double(), dim=-1)
    assert float((n.double() * radial).sum(-1).min()) > 0.9


def test_coincident_points_give_zeros():
    """40 copies of one point, k = 16: every neighbour of a copy is a copy -- zeros there, finite unit normals elsewhere."""
    from pnpp_hip import normals
    xyz = R.batch(("copies",), 64, R.SEED)
    x = _dev(xyz)
    n, curv, idx = normals.estimate_normals(x, 16, "centroid", curvature=True, neighbours=True)
    assert bool((idx[0, :40] < 40).all())
    assert bool((n[0, :40] == 0).all()) and bool((curv[0, :40] == 0).all())
    rest = n[0, 40:].double().norm(dim=-1)
    assert bool(torch.isfinite(n).all()) and bool(torch.isfinite(curv).all())
    assert float((rest - 1.0).abs().max()) <= R.NORM_GATE
    six = normals.with_normals(x, 16, "centroid")
    assert torch.equal(six[:, :, :3], x) and torch.equal(six[:, :, 3:], n)


RAGGED_LENS = [300, 17, 130]


@pytest.mark.parametrize("lengths_on", ["list", "device"])
@pytest.mark.parametrize("orient", ["centroid", None])
def test_ragged_rows_equal_the_cloud_alone(orient, lengths_on):
    from pnpp_hip import normals
    B, N, k = 3, 300, 16
    xyz = R.batch(("box", "cube", "sphere"), N, R.SEED + 3)
    for b, n in enumerate(RAGGED_LENS):
        xyz[b, n:] = np.nan                                                           # the padding may hold anything
    x = _dev(xyz)
    lengths = RAGGED_LENS if lengths_on == "list" else torch.tensor(RAGGED_LENS, dtype=torch.int32).cuda()
    n, curv, idx = normals.estimate_normals(x, k, orient, lengths=lengths, curvature=True, neighbours=True)
    six = normals.with_normals(x, k, orient, lengths=lengths)
    if orient == "centroid":
        ref = normals.reference_points(x, lengths)
        assert bool(torch.isfinite(ref).all())
    for b, nv in enumerate(RAGGED_LENS):
        alone = x[b:b + 1, :nv].contiguous()
        an, ac, ai = normals.estimate_normals(alone, k, orient, curvature=True, neighbours=True)
        assert torch.equal(n[b:b + 1, :nv], an) and torch.equal(curv[b:b + 1, :nv], ac) and torch.equal(idx[b:b + 1, :nv], ai), b
        assert torch.equal(six[b:b + 1, :nv, 3:], an) and torch.equal(six[b:b + 1, :nv, :3], alone), b
        if orient == "centroid":   # both are float64 sums rounded once to float32
            assert float((ref[b:b + 1] - normals.reference_points(alone)).abs().max()) <= 1e-7 * (100.0 if b == 0 else 1.0), b
        # every padding row is exact zeros in every column written
        assert bool((n[b, nv:] == 0).all()) and bool((curv[b, nv:] == 0).all()) and bool((idx[b, nv:] == 0).all()), b
        assert bool((six[b, nv:] == 0).all()), b


@pytest.mark.parametrize("N", [200, 1100])
def test_full_lengths_equal_the_uniform_call(N):
    from pnpp_hip import normals
    x = _dev(R.batch(("cube", "box"), N, R.SEED + 5))
    full = torch.full((2,), N, dtype=torch.int32).cuda()
    a = normals.estimate_normals(x, 16, "centroid", curvature=True, neighbours=True)
    b = normals.estimate_normals(x, 16, "centroid", lengths=full, curvature=True, neighbours=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(normals.with_normals(x, 16, "centroid"), normals.with_normals(x, 16, "centroid", lengths=full))


def test_two_tile_ragged_workgroups_beyond_the_cloud():
    """A padded N of two tiles with one cloud of a single tile and one that ends inside the second: whole workgroups lie beyond."""
    from pnpp_hip import normals
    N, lens = 1100, [1100, 70]
    xyz = R.batch(("sphere", "cube"), N, R.SEED + 9)
    xyz[1, 70:] = np.nan
    x = _dev(xyz)
    n, curv = normals.estimate_normals(x, 16, "centroid", lengths=lens, curvature=True)
    for b, nv in enumerate(lens):
        an, ac = normals.estimate_normals(x[b:b + 1, :nv].contiguous(), 16, "centroid", curvature=True)
        assert torch.equal(n[b:b + 1, :nv], an) and torch.equal(curv[b:b + 1, :nv], ac)
        assert bool((n[b, nv:] == 0).all()) and bool((curv[b, nv:] == 0).all())


def test_viewpoint_per_cloud_and_refusals():
    from pnpp_hip import normals
    x = _dev(R.batch(("cube", "sphere"), 64, R.SEED))
    views = torch.tensor([[0.5, 0.5, 9.0], [0.0, -9.0, 0.0]]).cuda()
    both = normals.estimate_normals(x, 8, views)
    for b in range(2):
        assert torch.equal(both[b:b + 1], normals.estimate_normals(x[b:b + 1].contiguous(), 8, views[b]))
    with pytest.raises(ValueError, match="viewpoint"):
        normals.estimate_normals(x, 8, torch.zeros(3, 3).cuda())
    with pytest.raises(ValueError, match="orient"):
        normals.estimate_normals(x, 8, "outward")
    with pytest.raises(ValueError, match="outside the supported range"):
        normals.estimate_normals(x, 2)
    with pytest.raises(RuntimeError, match="out of range"):
        normals.estimate_normals(x, 65)
    with pytest.raises(ValueError, match="lengths"):
        normals.estimate_normals(x, 8, lengths=[64, 7])                               # a cloud shorter than k, seen on the host


def test_graph_capture_and_replay():
    """lengths on the device, orient 'centroid': nothing is read back, so the call records into a graph; replays on new inputs
    (and new lengths) equal the eager call."""
    from pnpp_hip import normals
    N, k = 200, 16
    data = [R.batch(("cube", "box"), N, R.SEED + s) for s in (11, 12, 13)]
    lens = [[200, 200], [200, 150], [64, 200]]
    x = _dev(data[0]).clone()
    ln = torch.tensor(lens[0], dtype=torch.int32).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        normals.with_normals(x, k, "centroid", lengths=ln)                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = normals.with_normals(x, k, "centroid", lengths=ln)
    for d, l in zip(data[1:], lens[1:]):
        x.copy_(_dev(d))
        ln.copy_(torch.tensor(l, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, normals.with_normals(x, k, "centroid", lengths=ln))


# ---- end to end: bank -> loader -> augment -> classifier ---------------------------------------------------------------------------
def _bank(seed=5):
    from dataloader_common import DeviceCloudBank
    clouds = [R.FAMILIES[f](400 + 37 * i, R.SEED + 20 + i) for i, f in enumerate(("cube", "sphere", "cube", "sphere") * 2)]
    return DeviceCloudBank(clouds, "cuda", seed=seed)


def test_loader_feeds_the_classifier():
    from dataloader_common import BankLoader
    from models import get_loss
    from models.pointnet_pp_cls import PointNetPlusPlusCls
    labels = torch.arange(8) % 4
    plain = next(iter(BankLoader(_bank(), [labels], num_points=300, batch=4, shuffle=True, seed=3)))
    batch = next(iter(BankLoader(_bank(), [labels], num_points=300, batch=4, shuffle=True, seed=3, normals=16, channels_first=True)))
    x, y = batch
    assert x.shape == (4, 6, 300) and x.dtype == torch.float32 and x.is_cuda
    assert torch.equal(x[:, :3].transpose(1, 2), plain[0]) and torch.equal(y, plain[1])   # same seed, same draw: the same points
    nrm = x[:, 3:].transpose(1, 2).double().norm(dim=-1)
    assert float((nrm - 1.0).abs().max()) <= R.NORM_GATE
    torch.manual_seed(2)
    m = PointNetPlusPlusCls(num_classes=4, sa1=(64, 0.2, 32), sa2=(16, 0.4, 64)).cuda().train()
    loss = get_loss()(m(x), y.cuda())
    loss.backward()
    assert torch.isfinite(loss.detach()).item()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_augment_turns_the_normals_with_the_cloud():
    from dataloader_common import BankLoader
    from pnpp_hip.augment import Augment
    labels = torch.arange(8) % 4
    aug = Augment(seed=17)
    still = next(iter(BankLoader(_bank(), [labels], 300, 4, shuffle=False, normals=16)))[0]
    turned = next(iter(BankLoader(_bank(), [labels], 300, 4, shuffle=False, normals=16, augment=aug, kinds=("keep",))))[0]
    assert still.shape == turned.shape == (4, 300, 6)
    c, s = (aug.last_params[:, i].cpu().numpy().astype(np.float32)[:, None] for i in (0, 1))
    v = still.cpu().numpy()
    for col in (0, 3):   # the kernel's own float32 rotation about +Y, of the points and of the normals alike
        x0, y0, z0 = v[:, :, col], v[:, :, col + 1], v[:, :, col + 2]
        want = np.stack([c * x0 + s * z0, y0, c * z0 - s * x0], axis=-1).astype(np.float64)
        got = turned[:, :, col:col + 3].cpu().numpy().astype(np.float64)
        assert np.abs(got - want).max() <= 2e-7, col
    assert float(np.abs(s).min()) > 0.0   # every cloud was in fact turned
