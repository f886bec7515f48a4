"""Bit-identity of the store policy (pnpp_set_store_policy): write-through stores change how bytes leave the chip, never which bytes.

Every kernel that takes a policy writes the same values in the same order under every mask, so a level's forward and backward pass must
give torch.equal results under mask 0 and under a mask with every class on -- no tolerance, no case left out.  Each case runs one
set-abstraction level at the smallest shape its dispatcher still sends to the kernels in question (tests/dispatch.py asserts which ran):

  case        level                                                     rows   kernels with a policy (split form | float32-MFMA form)
  sa1         2 clouds x 256 points, 128 centres, k 32, 64-64-128       8192   gemm_wsf03 | gemm_wsf0*, gemm_wsf3<64> | gemm_wsf,
                                                                               gemm_wsd3<128,A5> | gemm_wsp, gemm_wsx
  sa2         8 clouds x 128 points, 32 centres, k 32, 128-128-256      8192   gather_rel_stats, gemm_wsf3<128> | gemm_wsf, pool_bwd,
                                                                               gemm_wsd3<256,A5> | gemm_wsq, gemm_wsd3<128,A4> | gemm_ws*
  sa1-ragged  2 clouds x 256 points, 129 centres                        8256   as sa1: 258 strips are no multiple of the waves in flight
  sa2-ragged  6 clouds x 128 points, 43 centres                         8256   as sa2
  sa3         group_all, 32 clouds x 32 points, 256-512-1024            1024   gemm_mid3 | gemm_mid (512 -> 1024), da_dw_mid (1024 -> 512), da_dw
  sa1-small   1 cloud x 1024 points, 128 centres, k 32, 64-64-128       4096   dw_xyz (layer 0 on raw coordinates, below the wave-strip band)
  sa2-small   5 clouds x 128 points, 32 centres, k 32, 128-128-256      5120   dw_kernel (past the small-M band: no da_dw), pool_bwd
  knn_pair    2 clouds x 1024 points, 128 / 32 centres, k 32                   knn_pair_kernel's moment partials (pnpp_knn_pair; the levels
                                                                               above search with knn_kernel, which writes none)
  (* takes no policy: it runs in the case but has nothing to compare.  gemm_wsq2_kernel, the PNPP_WSQ_FORM=2 form, and the
   stand-alone dw_lds_kernel take none either.)

Compared, all with torch.equal: the pooled output and its arg-max rows, the ReLU decisions of every layer, the running statistics, the
feature gradient (dA), every weight gradient (dW after its reduction launch) and every d-gamma / d-beta.  The stored activations Z
themselves are not read back (the level keeps them in a workspace with uninitialised padding); they are held through what reads them:
the sign of every element after BatchNorm (the ReLU decisions), their float64 column sums and sums of squares (the running statistics
after the finalisation launch), the next layer's product (the pooled output) and the backward sums over Z (d-gamma, dW).
Each case runs twice in a row with different inputs and compares both runs: a store that reached memory late would show as the first
run's values in the second.  The masks compared with 0: every class on (7) and, where it differs, the mask the library ships with.
"""
import pytest
import torch

from dispatch import expect, record

pytestmark = pytest.mark.gpu

ALL = 7
# (S, K, D, mlp, N, B)
SA1, SA1R = (128, 32, 0, [64, 64, 128], 256, 2), (129, 32, 0, [64, 64, 128], 256, 2)
SA2, SA2R = (32, 32, 128, [128, 128, 256], 128, 8), (43, 32, 128, [128, 128, 256], 128, 6)
SA3 = (None, None, 256, [256, 512, 1024], 32, 32)

WS1 = {"split": ["gemm_wsf03_kernel", "gemm_wsf3_kernel<64", "gemm_wsd3_kernel<128,32,A5>", "gemm_wsx_kernel<64,1,S3>", "xyz0_post_kernel"],
       "mfma": ["gemm_wsf0_kernel", "gemm_wsf_kernel<64,2", "gemm_wsp_kernel", "gemm_wsx_kernel<64,1>", "xyz0_post_kernel"]}
WS2 = {"split": ["gather_rel_stats_kernel", "gemm_wsf3_kernel<128", "pool_bwd_kernel", "gemm_wsd3_kernel<256,32,A5>", "gemm_wsd3_kernel<128,32,A4>"],
       "mfma": ["gather_rel_stats_kernel", "gemm_wsf_kernel<128,2", "pool_bwd_kernel", "gemm_wsq_kernel<256"]}
MID = {"split": ["gemm_mid3_kernel M=1024 N=1024", "da_dw_mid_kernel M=1024", "da_dw_kernel M=1024"],
       "mfma": ["gemm_mid_kernel M=1024 N=1024", "da_dw_mid_kernel M=1024", "da_dw_kernel M=1024"]}
SA1S, SA2S = (128, 32, 0, [64, 64, 128], 1024, 1), (32, 32, 128, [128, 128, 256], 128, 5)
SMALL1 = {f: ["dw_xyz_kernel"] for f in ("split", "mfma")}
SMALL2 = {f: ["dw_kernel<", "pool_bwd_kernel"] for f in ("split", "mfma")}
CASES = {"sa1": (SA1, 8192, WS1), "sa2": (SA2, 8192, WS2), "sa1-ragged": (SA1R, 8256, WS1), "sa2-ragged": (SA2R, 8256, WS2), "sa3": (SA3, 1024, MID),
         "sa1-small": (SA1S, 4096, SMALL1), "sa2-small": (SA2S, 5120, SMALL2)}


@pytest.fixture()
def knobs():
    from pnpp_hip import ops
    products, policy = ops.get_float32_products(), ops.get_store_policy()
    yield ops
    ops.set_float32_products(products)
    ops.set_store_policy(policy)


def _inputs(geo, seed):
    S, K, D, mlp, N, B = geo
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, N, 3, generator=g) * 2 - 1
    pts = None
    if D:
        pts = torch.randn(B, N, D, generator=g)
        if S is None:   # the level below hands on max-pooled ReLU activations
            pts = pts.abs()
    centres = None if S is None else torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)])
    gy = torch.randn(B, 1 if S is None else S, mlp[-1], generator=g)
    return xyz.cuda(), None if pts is None else pts.cuda(), None if centres is None else centres.cuda(), gy.cuda()


def _module(geo, seed):
    from models.pointnet_pp_8dir import PointNetSetAbstraction
    S, K, D, mlp, _, _ = geo
    torch.manual_seed(seed)
    sa = PointNetSetAbstraction(S, K, D, list(mlp), group_all=S is None)
    with torch.no_grad():
        for bn in sa.bns:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
    return sa.cuda().train()


def _step(ops, sa, inputs):
    """one forward + backward of the level; everything observable, cloned (the taps are views into the call's workspace)"""
    xyz, pts, centres, gy = inputs
    sa.zero_grad()
    pts = None if pts is None else pts.clone().requires_grad_(True)
    ops.sa_tap = []
    try:
        _, y = sa(xyz, pts, centres)
        tap = ops.sa_tap[0]
    finally:
        ops.sa_tap = None
    out = {"out": y.detach().clone(), "argmax": tap["argmax"].clone()}
    for l, m in enumerate(tap["relu_masks"]):
        out[f"relu_{l}"] = m.clone()
    y.backward(gy)
    torch.cuda.synchronize()
    if pts is not None:
        out["d_points"] = pts.grad.clone()
    for name, p in sa.named_parameters():
        out["d_" + name] = p.grad.clone()
    for l, bn in enumerate(sa.bns):
        out[f"rm_{l}"], out[f"rv_{l}"] = bn.running_mean.clone(), bn.running_var.clone()
    return out


def _two_runs(ops, geo, seed, mask):
    """a fresh copy of the level (same parameters), two steps in a row on different inputs under `mask`"""
    ops.set_store_policy(mask)
    assert ops.get_store_policy() == mask
    sa = _module(geo, seed)
    return [_step(ops, sa, _inputs(geo, seed + 1)), _step(ops, sa, _inputs(geo, seed + 2))]


@pytest.mark.parametrize("form", ["split", "mfma"])
@pytest.mark.parametrize("cid", list(CASES))
def test_results_do_not_depend_on_the_store_policy(knobs, cid, form):
    from pnpp_hip import _lib
    geo, rows, present = CASES[cid]
    S, K, D, mlp, N, B = geo
    assert B * (S or 1) * (K or N) == rows
    shipped = knobs.get_store_policy()
    knobs.set_float32_products(form)
    seed = 4200 + rows + len(cid)
    ref = {}
    tags = record(lambda: ref.update(r=_two_runs(knobs, geo, seed, 0)))
    expect(tags, present[form])
    for mask in sorted({ALL, shipped} - {0}):
        got = _two_runs(knobs, geo, seed, mask)
        for run, (r, g) in enumerate(zip(ref["r"], got)):
            assert r.keys() == g.keys()
            bad = [k for k in r if not torch.equal(r[k], g[k])]
            assert not bad, f"{cid} {form} mask {mask} run {run}: differs from mask 0 in {bad}"
    # the two runs had different inputs: a comparison of equal garbage would show here
    assert not torch.equal(ref["r"][0]["out"], ref["r"][1]["out"])
    assert _lib.lib().pnpp_debug_wsd3_timeouts() == 0


def _knn_pair(xyz, c1, c2, k):
    """pnpp_knn_pair with moments: both levels' neighbour lists and centres, and the moment partials it wrote"""
    from pnpp_hip import _lib as L
    lib = L.lib()
    B, N, _ = xyz.shape
    S1, S2 = c1.shape[1], c2.shape[1]
    idx1 = torch.full((B, S1, k), -1, dtype=torch.int32, device="cuda")
    idx2 = torch.full((B, S2, k), -1, dtype=torch.int32, device="cuda")
    a1, a2 = torch.zeros(B, S1, 3, device="cuda"), torch.zeros(B, S2, 3, device="cuda")
    nparts = lib.pnpp_knn_pair_partials(B, S1, N)
    mom = torch.zeros(nparts, 16, dtype=torch.float64, device="cuda")
    L.check(lib.pnpp_knn_pair(xyz.data_ptr(), B, N, c1.data_ptr(), S1, k, idx1.data_ptr(), a1.data_ptr(), c2.data_ptr(), S2, k,
                              idx2.data_ptr(), a2.data_ptr(), mom.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return {"idx1": idx1, "centres1": a1, "idx2": idx2, "centres2": a2, "moments": mom[:, :9].clone()}


def test_knn_pair_moments_do_not_depend_on_the_store_policy(knobs):
    B, N, S1, S2, k = 2, 1024, 128, 32, 32

    def two_runs(mask):
        knobs.set_store_policy(mask)
        out = []
        for seed in (77, 78):
            g = torch.Generator().manual_seed(seed)
            xyz = (torch.rand(B, N, 3, generator=g) * 2 - 1).cuda()
            c1 = torch.stack([torch.randperm(N, generator=g)[:S1] for _ in range(B)]).int().cuda()
            c2 = torch.stack([torch.randperm(S1, generator=g)[:S2] for _ in range(B)]).int().cuda()
            out.append(_knn_pair(xyz, c1, c2, k))
        return out

    ref = {}
    tags = record(lambda: ref.update(r=two_runs(0)))
    expect(tags, ["knn_pair_kernel"])
    for mask in sorted({ALL, knobs.get_store_policy() | 2} - {0}):   # bit 2: the class the moment partials belong to
        for run, (r, g) in enumerate(zip(ref["r"], two_runs(mask))):
            bad = [key for key in r if not torch.equal(r[key], g[key])]
            assert not bad, f"mask {mask} run {run}: differs from mask 0 in {bad}"
    assert float(ref["r"][0]["moments"].abs().sum()) > 0 and not torch.equal(ref["r"][0]["moments"], ref["r"][1]["moments"])


def test_setter_rejects_unknown_bits(knobs):
    from pnpp_hip import _lib
    before = knobs.get_store_policy()
    for bad in (-1, 8, 1 << 20):
        assert _lib.lib().pnpp_set_store_policy(bad) == _lib.PNPP_ERR_ARG
        assert knobs.get_store_policy() == before
    for mask in range(8):
        knobs.set_store_policy(mask)
        assert knobs.get_store_policy() == mask
