"""GPU parity, the front of the step: both levels' neighbour searches in one launch (knn_pair_kernel) and the moments of SA1's relative
coordinates that launch now sums on the way (they used to be rel_moments_kernel's, a launch of its own).

Search: idx of both levels and the written centres are bit-identical to the CPU reference tests/test_gpu_index.py uses
(oracle.knn_indices: the float32 restatement of square_distance + topk, ascending (distance, index)).

Moments: the nine totals (sum rel, sum rel rel^T) against a float64 CPU sum of the same float32 terms (rel by float32 subtraction, products
in float32).  Both sides add the same n <= 131,072 float32 terms in float64, in different orders: each addition rounds by at most 2^-53 of
the running sum, so the totals differ by at most n x 2^-53 ~ 1.5e-11 of sum |term|; the bound asserted is 1e-10 x sum |term| per moment.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# id -> (N, S1, k1, S2, k2, cloud): level 2 searches k2 among level 1's S1 centres
CASES = {
    "bench-geometry": (1024, 128, 32, 32, 32, "rand"),            # the benchmark's own geometry, small batch; level 2 fills the small form
    "second-tile-of-one": (1025, 6, 32, 3, 4, "rand"),            # second tile of one point; inactive waves in the last workgroup
    "tail-lanes": (130, 5, 32, 2, 5, "rand"),                     # tail lanes
    "level2-past-small-form": (300, 130, 32, 5, 32, "rand"),      # level 2: one candidate past the small form's 128
    "k64": (128, 8, 64, 4, 8, "rand"),                            # k = 64 bound
    "k65": (128, 8, 65, 4, 8, "rand"),                            # k > 64 path
    "all-equal": (256, 8, 32, 4, 8, "equal"),                     # all points equal: every key ties on the distance word, the pool is full
    "all-equal-overflow": (300, 8, 32, 4, 8, "equal"),            # ... and more keys than the pool holds: the fallback
    "level2-tile-not-pow2": (777, 96, 32, 40, 32, "rand"),        # level-2 gather, S1 = 96
    "s-not-multiple-of-8": (512, 13, 32, 7, 13, "rand"),          # S1 % 4 != 0 and an odd number of four-query groups
    "duplicates": (200, 10, 16, 4, 10, "dups"),                   # exact ties between distinct rows: lowest index wins
    "all-equal-two-tiles": (1100, 8, 32, 4, 8, "equal"),          # the fallback on the first tile, then a second tile with the previous list riding along
}
B = 2


def _cloud(N, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "equal":
        return torch.full((B, N, 3), 0.37)
    if kind == "dups":
        base = torch.rand(B, 40, 3, generator=g)
        return torch.stack([base[b, torch.randint(0, 40, (N,), generator=g)] for b in range(B)])
    return torch.rand(B, N, 3, generator=g) * 2 - 1


def _lib():
    from pnpp_hip import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.lib(), _lib


def _pair(xyz, c1, k1, c2, k2, with_moments=True):
    """pnpp_knn_pair on device copies -> idx1, centres1, idx2, centres2, moment partials (rows beyond the written ones stay NaN)"""
    lib, L = _lib()
    Bq, N, _ = xyz.shape
    S1, S2 = c1.shape[1], c2.shape[1]
    x, d1, d2 = xyz.cuda().contiguous(), c1.int().cuda().contiguous(), c2.int().cuda().contiguous()
    idx1 = torch.full((Bq, S1, k1), -1, dtype=torch.int32, device="cuda")
    idx2 = torch.full((Bq, S2, k2), -1, dtype=torch.int32, device="cuda")
    a1 = torch.full((Bq, S1, 3), float("nan"), device="cuda")
    a2 = torch.full((Bq, S2, 3), float("nan"), device="cuda")
    nparts = lib.pnpp_knn_pair_partials(Bq, S1, N)
    mom = torch.full((nparts + 2, 16), float("nan"), dtype=torch.float64, device="cuda")
    L.check(lib.pnpp_knn_pair(x.data_ptr(), Bq, N, d1.data_ptr(), S1, k1, idx1.data_ptr(), a1.data_ptr(), d2.data_ptr(), S2, k2,
                              idx2.data_ptr(), a2.data_ptr(), mom.data_ptr() if with_moments else None,
                              torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return idx1.cpu(), a1.cpu(), idx2.cpu(), a2.cpu(), mom.cpu(), nparts


@pytest.fixture(scope="module")
def cases(oracle):
    """every case's inputs, CPU reference and device result, computed once"""
    out = {}
    for i, (name, (N, S1, k1, S2, k2, kind)) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(100 + i)
        xyz = _cloud(N, kind, 7 + i)
        c1 = torch.stack([torch.randperm(N, generator=g)[:S1] for _ in range(B)])
        c2 = torch.stack([torch.randperm(S1, generator=g)[:S2] for _ in range(B)])
        new1 = oracle.index_points(xyz, c1)
        new2 = oracle.index_points(new1, c2)
        ref1, ref2 = oracle.knn_indices(new1, xyz, k1), oracle.knn_indices(new2, new1, k2)
        out[name] = dict(xyz=xyz, c1=c1, c2=c2, new1=new1, new2=new2, ref1=ref1, ref2=ref2, got=_pair(xyz, c1, k1, c2, k2))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_search_bit_identical(cases, name):
    c = cases[name]
    idx1, a1, idx2, a2, _, _ = c["got"]
    assert np.array_equal(idx1.numpy(), c["ref1"].numpy().astype(np.int32))
    assert np.array_equal(idx2.numpy(), c["ref2"].numpy().astype(np.int32))
    assert a1.numpy().tobytes() == c["new1"].contiguous().numpy().tobytes()
    assert a2.numpy().tobytes() == c["new2"].contiguous().numpy().tobytes()


def _moment_reference(xyz, new1, idx):
    """nine float64 totals of float32 terms, and sum |term| of each"""
    rel = _gather(xyz, idx) - new1[:, :, None, :]                       # float32 subtraction
    x, y, z = rel[..., 0], rel[..., 1], rel[..., 2]
    terms = [x, y, z, x * x, x * y, x * z, y * y, y * z, z * z]               # float32 products
    return (np.array([t.double().sum().item() for t in terms]), np.array([t.double().abs().sum().item() for t in terms]))


def _gather(xyz, idx):
    Bq, S, k = idx.shape
    return torch.gather(xyz, 1, idx.reshape(Bq, S * k, 1).long().expand(-1, -1, 3)).reshape(Bq, S, k, 3)


@pytest.mark.parametrize("name", list(CASES))
def test_moments_against_float64_sum(cases, name):
    c = cases[name]
    _, _, _, _, mom, nparts = c["got"]
    N, S1 = CASES[name][0], CASES[name][1]
    assert nparts in (B * ((S1 + 3) // 4), B * ((S1 + 7) // 8)), nparts          # one partial per level-1 search workgroup
    assert torch.isfinite(mom[:nparts, :9]).all(), "a search workgroup wrote no partial"
    assert torch.isnan(mom[nparts:]).all(), "more partials written than pnpp_knn_pair_partials reports"
    ref, mag = _moment_reference(c["xyz"], c["new1"], c["ref1"])
    got = mom[:nparts, :9].sum(0).numpy()
    err = np.abs(got - ref)
    print(f"{name}: nparts={nparts} max err / sum|term| = {float((err / np.maximum(mag, 1e-300)).max()):.3e}")
    assert (err <= 1e-10 * mag).all(), (got, ref, mag)


def test_search_without_moments_equals_search_with(cases):
    """the moment sums ride along: asking for them changes neither level's result"""
    c = cases["bench-geometry"]
    N, S1, k1, S2, k2, _ = CASES["bench-geometry"]
    plain = _pair(c["xyz"], c["c1"], k1, c["c2"], k2, with_moments=False)
    for i in range(4):
        assert plain[i].numpy().tobytes() == c["got"][i].numpy().tobytes()
    assert torch.isnan(plain[4]).all()


def _levels(seed=3):
    from models.pointnet_pp_8dir import PointNetSetAbstraction
    torch.manual_seed(seed)
    sa1 = PointNetSetAbstraction(128, 32, 0, [64, 64, 128]).cuda().train()
    sa2 = PointNetSetAbstraction(32, 32, 128, [128, 128, 256]).cuda().train()
    g = torch.Generator().manual_seed(11)
    xyz = (torch.rand(B, 1024, 3, generator=g) * 2 - 1).cuda()
    c1 = torch.stack([torch.randperm(1024, generator=g)[:128] for _ in range(B)]).cuda()
    c2 = torch.stack([torch.randperm(128, generator=g)[:32] for _ in range(B)]).cuda()
    return sa1, sa2, xyz, c1, c2


def test_two_runs_are_bitwise_equal(cases):
    """idx, moments and layer 0's statistics (its running mean / variance are pure functions of mean / istd) of two runs"""
    c = cases["bench-geometry"]
    N, S1, k1, S2, k2, _ = CASES["bench-geometry"]
    again = _pair(c["xyz"], c["c1"], k1, c["c2"], k2)
    for i in (0, 2):
        assert again[i].numpy().tobytes() == c["got"][i].numpy().tobytes()
    assert again[4][:again[5]].numpy().tobytes() == c["got"][4][:c["got"][5]].numpy().tobytes()
    from models.pointnet_pp_8dir import stacked_levels
    res = []
    for _ in range(2):
        sa1, sa2, xyz, c1, c2 = _levels()
        _, l1, _, l2 = stacked_levels(sa1, sa2, xyz, c1, c2)
        res.append((sa1.bns[0].running_mean.clone(), sa1.bns[0].running_var.clone(), l1.detach().clone(), l2.detach().clone()))
    for u, v in zip(*res):
        assert torch.equal(u, v)


def test_route_with_and_without_the_pair_search():
    """training-mode SA1 + SA2, B = 2.  Grouped by pnpp_sa_group_pair, SA1's forward records no rel_moments launch (the search summed the
    moments); on the per-level path (no pair search) it records one.  Layer 0's statistics of the two routes agree to float32 rounding: the
    same float32 terms, float64 sums in another order, so the float32 results can differ in the last place (2^-24 ~ 6e-8; 3e-7 asserted)."""
    from dispatch import record
    from models.pointnet_pp_8dir import stacked_levels
    res = {}
    for route in ("pair", "per-level"):
        sa1, sa2, xyz, c1, c2 = _levels()
        out = {}

        def fn():
            if route == "pair":
                out["l1"] = stacked_levels(sa1, sa2, xyz, c1, c2)[1]
            else:
                l1_xyz, out["l1"] = sa1(xyz, None, c1)
                sa2(l1_xyz, out["l1"], c2)
        res[route] = (record(fn), sa1.bns[0].running_mean.cpu().numpy(), sa1.bns[0].running_var.cpu().numpy())
    tags = res["pair"][0]
    assert not [t for t in tags if t.startswith("rel_moments_kernel")], tags
    assert [t for t in tags if t.startswith("knn_pair_kernel B=2 | S=128 N=1024 k=32 | S=32 N=128 k=32")], tags
    assert len([t for t in res["per-level"][0] if t.startswith("rel_moments_kernel")]) == 1, res["per-level"][0]
    for i in (1, 2):
        np.testing.assert_allclose(res["pair"][i], res["per-level"][i], rtol=3e-7, atol=1e-9)
