"""Pins the CPU oracle at the EDGES of the index primitives against tests/golden/index_edges.npz, which oracle/make_index_edges.py
captured from the reference's own functions: the radius query one float32 either side of float32(radius ** 2), its empty / under-full /
full lists, farthest-point sampling on duplicates, npoint > N and N = 1, square_distance of coincident points, kNN with k == N and
k == 1.  Bit for bit, no tolerances.  CPU only; the same entries run through the HIP kernels in tests/test_gpu_index_edges.py."""
import numpy as np
import pytest

import index_edges_cases as E


@pytest.mark.parametrize("r", E.RADII)
def test_ball_query_radius_boundary_matches_demo(oracle, golden, r):
    """Members are the points with !(d > float32(r ** 2)), r ** 2 formed in double (PointNet++Demo.py:65).  A radius squared after
    it was rounded to float32 fails here: a point at t + 1 ulp admitted for 0.05, 0.1, 0.2, 0.4, 0.8, one at t rejected for 0.35, 0.45."""
    xyz, new_xyz, lists = E.boundary(golden(E.FIXTURE), r)
    for nsample, want in lists:
        got = oracle.ball_query(r, nsample, xyz, new_xyz).numpy()
        assert np.array_equal(got, want), (r, nsample, got.tolist(), want.tolist())


@pytest.mark.parametrize("r", E.RADII)
def test_float32_radius_rule_is_the_references_only_where_documented(oracle, golden, r):
    """oracle.ball_query_float32_radius restates the C entries that take a float32 radius (include/pnpp_hip.h): the reference's
    lists for 0.25 and 0.3, one boundary value off for the other radii."""
    xyz, new_xyz, lists = E.boundary(golden(E.FIXTURE), r)
    nsample, reference = lists[0]
    got = oracle.ball_query_float32_radius(r, nsample, xyz, new_xyz).numpy()
    assert np.array_equal(got, reference) == (r in (0.25, 0.3))


def test_radius_boundary_fixture_has_teeth(golden):
    """From the fixture alone: for every radius a stored candidate at d == t is in the reference's list, one at d == t + 1 ulp is not,
    and the two values either side are there too -- so a threshold one float32 off in either direction changes some list."""
    g = golden(E.FIXTURE)
    assert tuple(g["rb_radii"].tolist()) == E.RADII
    for r, t_bits in zip(E.RADII, g["rb_t_bits"].tolist()):
        assert int(np.float32(r ** 2).view(np.uint32)) == t_bits
        d_bits, idx = g[f"rb_{r}_bits"].astype(np.int64), g[f"rb_{r}_idx"]
        M = d_bits.shape[0]
        assert idx.shape == (1, 1, M)                          # nsample == the number of candidates: nothing was cut off
        members = set(idx.ravel().tolist())
        at = lambda k: set(np.flatnonzero(d_bits == t_bits + k).tolist())
        assert len(at(-1)) >= 1 and len(at(0)) >= 1 and len(at(1)) >= 1 and len(at(2)) >= 1, r
        assert at(0) & members, r
        assert at(1) - members, r
        assert at(-1) <= members and at(0) <= members and not (at(1) | at(2)) & members, r
        cut = g[f"rb_{r}_idx_cut"]
        assert cut.shape[-1] < len(members) and np.array_equal(cut.ravel(), sorted(members)[:cut.shape[-1]])   # first in index order


def test_threshold_entry_points_without_gpu(golden):
    """pnpp_ball_query_r2 / _r2_ragged are bound with a C float for the threshold -- the one rounding of the python float r ** 2 that
    ops.ball_query relies on gives the fixture's bits -- and refuse bad arguments before any launch, the ragged one a null lengths."""
    import ctypes
    from pnpp_hip import build, _lib
    build.build()
    lib = _lib.lib()
    g = golden(E.FIXTURE)
    assert _lib.SIGNATURES["pnpp_ball_query_r2"][1][5] is ctypes.c_float and _lib.SIGNATURES["pnpp_ball_query_r2_ragged"][1][6] is ctypes.c_float
    for r, t_bits in zip(E.RADII, g["rb_t_bits"].tolist()):
        assert int(np.float32(ctypes.c_float(float(r) ** 2).value).view(np.uint32)) == t_bits
    ptr = 4096                                                 # a non-null "device pointer": refused before anything could read it
    assert lib.pnpp_ball_query_r2(None, None, 1, 1, 1, 0.04, 1, None, None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_ball_query_r2(ptr, ptr, 1, 1, 1, 0.04, 0, ptr, None) == _lib.PNPP_ERR_ARG
    assert lib.pnpp_ball_query_r2_ragged(ptr, ptr, 2, 4, 64, None, 0.04, 8, ptr, None) == _lib.PNPP_ERR_ARG
    assert b"null lengths" in lib.pnpp_last_error()


@pytest.mark.parametrize("tag,r", E.OTHER_BALL)
def test_ball_query_empty_underfull_full_match_demo(oracle, golden, tag, r):
    xyz, new_xyz, nsample, want = E.other_ball(golden(E.FIXTURE), tag)
    N = xyz.shape[1]
    if tag == "be_empty":
        assert (want == N).all()
    elif tag == "be_under":
        assert any(1 < len(set(row.tolist())) < nsample and row[-1] == row[0] for row in want.reshape(-1, nsample))
    else:
        assert nsample == N and (want == np.arange(N)).all()
    assert np.array_equal(oracle.ball_query(r, nsample, xyz, new_xyz).numpy(), want)


@pytest.mark.parametrize("tag", E.FPS)
def test_fps_duplicates_overdraw_single_point_match_demo(oracle, golden, tag):
    xyz, npoint, start, want = E.fps(golden(E.FIXTURE), tag)
    assert np.array_equal(oracle.farthest_point_sample(xyz, npoint, start.numpy()).numpy(), want)


def test_square_distance_of_coincident_points_bit_exact(oracle, golden):
    g = golden(E.FIXTURE)
    xyz = g["sqself_xyz"]
    got = oracle.square_distance(xyz, xyz).numpy()
    assert got.view(np.uint32).tobytes() == g["sqself_bits"].tobytes()
    diag = g["sqself_bits"].view(np.float32)[:, np.arange(40), np.arange(40)]
    assert (diag < 0).any()                                    # the diagonal is rounding residue, not zero


def test_knn_whole_cloud_and_single_neighbour_match_reference(oracle, golden):
    g = golden(E.FIXTURE)
    xyz, new_xyz = E._t(g["kq_xyz"]), E._t(g["kq_new_xyz"])
    for k in (33, 1):
        got = oracle.knn_indices(new_xyz, xyz, k).numpy()
        assert np.array_equal(np.sort(got, -1), g[f"kq_idx{k}_sorted"])
