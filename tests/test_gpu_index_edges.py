"""GPU parity at the EDGES of the index kernels.

Part 1: the entries of tests/golden/index_edges.npz -- inputs and the REFERENCE's own outputs (oracle/make_index_edges.py) -- through
ops.ball_query (uniform and ragged), ops.farthest_point_sample, ops.square_distance and ops.knn, and the radius-boundary clouds through
the model surface that calls ops.ball_query.  Part 2: the structural edges of ball_query_kernel (lane chunks of 64, BALL_TILE = 1024,
four waves per workgroup, the fill loop, early exit) against the CPU oracle, which tests/test_index_edges_cpu.py pins to the same fixture.
np.array_equal / byte equality throughout: there are no tolerances.  Reads tests/golden/ and oracle/ only."""
import numpy as np
import pytest
import torch

import index_edges_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from pnpp_hip import ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return ops


def _ball(ops, r, nsample, xyz, new_xyz, lengths=None):
    return ops.ball_query(r, nsample, xyz.cuda(), new_xyz.cuda(), lengths=lengths).cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------ part 1: the reference's own outputs
@pytest.mark.parametrize("r", E.RADII)
def test_ball_query_radius_boundary_matches_demo(ops, golden, r):
    """d == t - 1 ulp, t (members) and t + 1 ulp, t + 2 ulp (not), t = float32(r ** 2) as PointNet++Demo.py:65 forms it; then the
    list cut short (ascending index order).  Ragged: the same lists with NaN rows beyond the length."""
    xyz, new_xyz, lists = E.boundary(golden(E.FIXTURE), r)
    padded, lengths = E.nan_padded(xyz)
    for nsample, want in lists:
        got = _ball(ops, r, nsample, xyz, new_xyz)
        assert np.array_equal(got, want), (r, nsample, got.tolist(), want.tolist())
        got = _ball(ops, r, nsample, padded, new_xyz, lengths)
        assert np.array_equal(got, want), ("ragged", r, nsample, got.tolist(), want.tolist())


@pytest.mark.parametrize("r", E.RADII)
def test_float32_radius_entries_keep_their_documented_rule(ops, oracle, golden, r):
    """pnpp_ball_query / pnpp_ball_query_ragged, which nothing in the library calls any more, take the radius as a float32 and square
    it afterwards (include/pnpp_hip.h).  On the boundary clouds that is the reference's list for 0.25 and 0.3 only."""
    from pnpp_hip import _lib as L
    xyz, new_xyz, lists = E.boundary(golden(E.FIXTURE), r)
    nsample, reference = lists[0]
    want = oracle.ball_query_float32_radius(r, nsample, xyz, new_xyz).numpy()
    assert np.array_equal(want, reference) == (r in (0.25, 0.3))
    padded, lengths = E.nan_padded(xyz)
    x, xp, c = xyz.cuda(), padded.cuda(), new_xyz.cuda()
    dev_lengths = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    idx = torch.empty(1, 1, nsample, dtype=torch.int32, device="cuda")
    L.check(L.lib().pnpp_ball_query(c.data_ptr(), x.data_ptr(), 1, 1, x.shape[1], r, nsample, idx.data_ptr(), ops._stream()))
    assert np.array_equal(idx.cpu().numpy(), want)
    idx.zero_()
    L.check(L.lib().pnpp_ball_query_ragged(c.data_ptr(), xp.data_ptr(), 1, 1, xp.shape[1], dev_lengths.data_ptr(), r, nsample,
                                           idx.data_ptr(), ops._stream()))
    assert np.array_equal(idx.cpu().numpy(), want)


@pytest.mark.parametrize("tag,r", E.OTHER_BALL)
def test_ball_query_empty_underfull_full_match_demo(ops, golden, tag, r):
    xyz, new_xyz, nsample, want = E.other_ball(golden(E.FIXTURE), tag)
    assert np.array_equal(_ball(ops, r, nsample, xyz, new_xyz), want)
    padded, lengths = E.nan_padded(xyz)
    assert np.array_equal(_ball(ops, r, nsample, padded, new_xyz, lengths), want)   # the empty fill is the length, here N


@pytest.mark.parametrize("tag", E.FPS)
def test_fps_duplicates_overdraw_single_point_match_demo(ops, golden, tag):
    xyz, npoint, start, want = E.fps(golden(E.FIXTURE), tag)
    assert np.array_equal(ops.farthest_point_sample(xyz.cuda(), npoint, start).cpu().numpy(), want)
    padded, lengths = E.nan_padded(xyz)
    assert np.array_equal(ops.farthest_point_sample(padded.cuda(), npoint, start, lengths=lengths).cpu().numpy(), want)


def test_square_distance_of_coincident_points_bit_exact(ops, golden):
    g = golden(E.FIXTURE)
    xyz = E._t(g["sqself_xyz"]).cuda()
    got = ops.square_distance(xyz, xyz).cpu().numpy()
    assert got.view(np.uint32).tobytes() == g["sqself_bits"].tobytes()


def test_knn_whole_cloud_and_single_neighbour_match_reference(ops, golden):
    g = golden(E.FIXTURE)
    xyz, new_xyz = E._t(g["kq_xyz"]).cuda(), E._t(g["kq_new_xyz"]).cuda()
    for k in (33, 1):
        got = ops.knn(new_xyz, xyz, k).cpu().numpy()
        assert np.array_equal(np.sort(got, -1), g[f"kq_idx{k}_sorted"])


@pytest.fixture
def neighbour_lists(ops, monkeypatch):
    """what a level hands to ops.set_abstraction as neighbour_idx: the level's own call of ops.ball_query is what runs, the MLP is not"""
    seen = []

    def record(xyz, points, centre, *args, neighbour_idx=None, **kwargs):
        seen.append(neighbour_idx)
        return None, None

    monkeypatch.setattr(ops, "set_abstraction", record)
    return seen


@pytest.mark.parametrize("r", [0.2, 0.4])
def test_classifier_levels_query_at_the_reference_threshold(ops, golden, neighbour_lists, r):
    """SimpleSetAbstraction (sa1: r = 0.2, sa2: r = 0.4) and ClsPredictor's neighbour-list step on the boundary cloud: the centre is a
    row of the cloud, so farthest-point sampling of one point from that start index selects it."""
    from models.pointnet_pp_cls import SimpleSetAbstraction
    from pnpp_hip.inference import ClsPredictor
    g = golden(E.FIXTURE)
    xyz, new_xyz, lists = E.boundary(g, r)
    ci = int(g[f"rb_{r}_centre_idx"])
    assert torch.equal(xyz[0, ci], new_xyz[0, 0])
    for nsample, want in lists:
        sa = SimpleSetAbstraction(npoint=1, radius=r, nsample=nsample, in_channel=0, mlp=[32, 32, 64])
        sa.rows(xyz.cuda(), None, start=torch.tensor([ci]))
        assert np.array_equal(neighbour_lists.pop().cpu().numpy(), want), (r, nsample)
        centre = torch.tensor([[ci]], dtype=torch.int32, device="cuda")
        got = ClsPredictor._neighbours(sa, xyz.cuda(), centre, None)
        assert np.array_equal(got.cpu().numpy(), want), ("predictor", r, nsample)


def test_set_abstraction_ball_grouper_queries_at_the_reference_threshold(ops, golden, neighbour_lists):
    from models.pointnet_pp_8dir import PointNetSetAbstraction
    g = golden(E.FIXTURE)
    xyz, new_xyz, lists = E.boundary(g, 0.2)
    ci = int(g["rb_0.2_centre_idx"])
    for nsample, want in lists:
        sa = PointNetSetAbstraction(1, nsample, 0, [32, 32, 64], grouper="ball:0.2")
        sa(xyz.cuda(), None, torch.tensor([[ci]], device="cuda"))
        assert np.array_equal(neighbour_lists.pop().cpu().numpy(), want), nsample


# ------------------------------------------------------------------------------------------ part 2: structural edges vs the oracle
def _counts(oracle, r, xyz, new_xyz):
    """members per centre, from the oracle's uncut list (padding repeats the first member; N marks an empty ball) -> (B,S)"""
    N = xyz.shape[1]
    full = oracle.ball_query(r, N, xyz, new_xyz).numpy()
    return np.array([[0 if row[0] == N else len(set(row.tolist())) for row in cloud] for cloud in full])


def _cube(seed, B, N):
    return torch.rand(B, N, 3, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_ball_query_lane_chunk_and_tile_edges(ops, oracle, N):
    """The cloud's LAST row sits alone, far from the rest, with a centre on it: its list is that one index, found in the last
    (partial) lane chunk of the last tile after nothing but misses.  The other centres have ordinary, cut and empty balls."""
    xyz = _cube(100 + N, 2, N)
    xyz[:, N - 1] = torch.tensor([5.0, 5.25, 5.5])
    picks = [N - 1, 0, N // 2, N // 3]
    new_xyz = torch.cat([xyz[:, picks], torch.full((2, 1, 3), -9.0)], 1).contiguous()
    r = min(0.5, (6.0 * 12 / (np.pi * N)) ** (1.0 / 3.0))          # about 12 members per ball inside the cube
    nsample = min(N, 16)
    want = oracle.ball_query(r, nsample, xyz, new_xyz).numpy()
    assert (want[:, 0] == N - 1).all() and (want[:, 4] == N).all()
    if N >= 63:
        cnt = _counts(oracle, r, xyz, new_xyz)
        assert (cnt[:, 1:4] >= 1).all() and (cnt[:, 1:4] > 1).any()   # the centre itself, and balls with real neighbours
    assert np.array_equal(_ball(ops, r, nsample, xyz, new_xyz), want)


@pytest.mark.parametrize("S", [1, 3, 4, 5])
def test_ball_query_inactive_waves_reach_the_barriers(ops, oracle, S):
    """four centres per workgroup: with S = 1, 3, 5 the last workgroup has waves without a centre; two tiles, so they pass barriers"""
    xyz = _cube(7, 3, 1100)
    new_xyz = xyz[:, 1090:1090 + S].contiguous()
    want = oracle.ball_query(0.15, 24, xyz, new_xyz).numpy()
    assert (want >= 1024).any() and (want < 1024).any()             # members in both tiles
    assert np.array_equal(_ball(ops, 0.15, 24, xyz, new_xyz), want)


def _clustered():
    """300 points: even rows in a cluster of diameter < 0.1 away from the rest, odd rows spread over a cube of side 4; centres on the
    cluster (a crowded ball), on spread points (sparse balls) and far away (an empty ball)"""
    g = torch.Generator().manual_seed(11)
    xyz = torch.empty(2, 300, 3)
    xyz[:, 0::2] = 5.0 + 0.05 * torch.rand(2, 150, 3, generator=g)
    xyz[:, 1::2] = 4.0 * torch.rand(2, 150, 3, generator=g) - 2.0
    new_xyz = torch.cat([xyz[:, [0, 1, 3, 5, 7, 150]], torch.full((2, 1, 3), 30.0)], 1).contiguous()
    return xyz, new_xyz


@pytest.mark.parametrize("nsample", [1, 5, 64, 65, 130])
def test_ball_query_fill_stride_and_count_crossing(ops, oracle, nsample):
    """Sparse balls at nsample > 64 + members: the fill loop runs more than one stride of 64.  The crowded ball has 150 members in
    rows 0, 2, 4 ...: 32 per lane chunk of 64, so the count crosses nsample = 5 inside the first chunk, reaches 64 at the end
    of the second, and crosses 65 and 130 inside the third and the fifth."""
    xyz, new_xyz = _clustered()
    r = 0.6
    cnt = _counts(oracle, r, xyz, new_xyz)
    assert (cnt[:, 0] == 150).all() and (cnt[:, -1] == 0).all()
    assert ((cnt[:, 1:5] >= 1) & (cnt[:, 1:5] < 60)).all()         # under-full wherever nsample >= 64, by more than 64 at 130
    want = oracle.ball_query(r, nsample, xyz, new_xyz).numpy()
    assert (want[:, 0] == 2 * np.arange(nsample)).all()             # the crowded ball, cut: the cluster's rows in index order
    assert (want[:, -1] == 300).all()
    assert np.array_equal(_ball(ops, r, nsample, xyz, new_xyz), want)


@pytest.mark.parametrize("nsample", [1, 64, 65, 130, 300])
def test_ball_query_everything_inside_is_arange(ops, oracle, nsample):
    xyz = _cube(13, 2, 300)
    new_xyz = xyz[:, :5].contiguous()
    want = oracle.ball_query(10.0, nsample, xyz, new_xyz).numpy()
    assert (want == np.arange(nsample)).all()
    assert np.array_equal(_ball(ops, 10.0, nsample, xyz, new_xyz), want)


def test_ball_query_first_hit_in_the_third_tile(ops, oracle):
    """N = 2049: row 2048 is the only member of the first centre's ball -- two tiles without a hit, then the first one in the third;
    the other three waves of its workgroup have their lists full after the first tile and only keep the barriers company."""
    xyz = _cube(17, 2, 2049)
    xyz[:, 2048] = torch.tensor([3.0, 3.0, 3.0])
    xyz[:, :40] = 0.5 + 0.01 * torch.rand(2, 40, 3, generator=torch.Generator().manual_seed(18))
    new_xyz = torch.stack([xyz[:, 2048] + 0.01, xyz[:, 0], xyz[:, 1], xyz[:, 2]], 1).contiguous()
    want = oracle.ball_query(0.2, 8, xyz, new_xyz).numpy()
    assert (want[:, 0] == 2048).all() and want[:, 0].min() >= 2048
    assert (want[:, 1:] == np.arange(8)).all()                      # full within the first lane chunk of the first tile
    assert np.array_equal(_ball(ops, 0.2, 8, xyz, new_xyz), want)


def test_ball_query_one_fewer_exact_and_one_more_member_than_nsample(ops, oracle):
    """nsample taken from the oracle's member count c of a ball: c + 1 (one slot padded), c (exactly full, nothing padded, nothing
    cut) and c - 1 (the last member cut)."""
    xyz = _cube(19, 1, 500)
    new_xyz = xyz[:, 100:108].contiguous()
    r = 0.2
    cnt = _counts(oracle, r, xyz, new_xyz)[0]
    s = int(np.argmax(cnt))
    c = int(cnt[s])
    assert c >= 3
    uncut = oracle.ball_query(r, c, xyz, new_xyz).numpy()[0, s]
    assert len(set(uncut.tolist())) == c
    for nsample in (c + 1, c, c - 1):
        want = oracle.ball_query(r, nsample, xyz, new_xyz).numpy()
        row = want[0, s]
        if nsample == c + 1:
            assert np.array_equal(row[:c], uncut) and row[c] == uncut[0]
        else:
            assert np.array_equal(row, uncut[:nsample])
        assert np.array_equal(_ball(ops, r, nsample, xyz, new_xyz), want)


def test_ball_query_many_small_clouds_in_one_launch(ops, oracle):
    xyz = _cube(23, 65, 70)
    new_xyz = torch.cat([xyz[:, [69, 0, 33]], torch.full((65, 1, 3), 8.0)], 1).contiguous()
    want = oracle.ball_query(0.3, 8, xyz, new_xyz).numpy()
    cnt = _counts(oracle, 0.3, xyz, new_xyz)
    assert (cnt[:, 3] == 0).all() and (cnt[:, :3] > 8).any() and ((cnt[:, :3] >= 1) & (cnt[:, :3] < 8)).any()
    assert len({row.tobytes() for row in want}) == 65               # every cloud's lists are its own
    assert np.array_equal(_ball(ops, 0.3, 8, xyz, new_xyz), want)
