"""The fused set-abstraction inference kernels (csrc/sa_infer_kernels.hip: sa_infer_kernel<64>, sa_infer_kernel<32>,
sa_infer_wide_kernel) at every band of infer_plan, far from the three model shapes: column-block counts that are no power of two,
K = 16 on the 32-row tile, the TM = 64 / 32 switch at its edge, layer-0 paddings other than 13 columns, Kd0 > C1, the largest LDS
tile the plan takes, every column split of the last layer, and the level searching its own neighbours.

Each case (tests/sa_infer_bands_cases.py) is one level through the C ABI -- fold, then one pnpp_sa_infer launch -- against
_level64(fold=True), the plain float64 evaluation of the same folded level.  Gate: relmax <= 1e-5, the level gate G2 of
tests/test_gpu_inference.py.  Besides: nothing is left unwritten (both outputs start as NaN), the guard groups behind the outputs
are bit-unchanged (the `g < G` / `g + 1 < G` stores), new_xyz is bit-equal to the gathered centres, and the recorded tag names the
kernel, TM and split the table expects, so a case fails when the plan moves instead of quietly measuring another band."""
import pytest
import torch

from conftest import has_gpu, relmax
from dispatch import field, find, record
from sa_infer_bands_cases import CASES
from test_gpu_pointnet_pp_cls import GUARD_FILL, _level64, _params64, _randomise, _sa_infer

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an AMD GPU")]

G2 = 1e-5
GUARD = 4   # groups behind the real ones: a 64-row tile of K = 16 holds 4


@pytest.mark.parametrize("case", list(CASES))
def test_sa_infer_band(case, request):
    from pnpp_hip import ops
    from models.pointnet_pp_cls import SimpleSetAbstraction, SimpleSetAbstractionGroupAll
    c = CASES[case]
    B, N, S, K, D, ch = c["B"], c["N"], c["S"], c["K"], c["D"], c["ch"]
    ga, radius, search = c.get("group_all", False), c.get("radius"), c.get("search", False)
    torch.manual_seed(31)   # the convolutions' own initialisation: every weight row and bias distinct
    level = SimpleSetAbstractionGroupAll(D, ch) if ga else SimpleSetAbstraction(S, radius or 1.0, K, D, ch)
    level = _randomise(level, 32).cuda().eval()
    g = torch.Generator().manual_seed(33)
    xyz = torch.rand(B, N, 3, generator=g).cuda()
    pts = torch.randn(B, N, D, generator=g).cuda() if D else None
    centre = nbr = idx_out = None
    if not ga:
        centre = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)]).to(torch.int32).cuda()
        if search:
            idx_out = torch.full((B, S, K), -1, dtype=torch.int32, device="cuda")
        elif radius is None:
            nbr = torch.randint(0, N, (B, S, K), generator=g).to(torch.int32).cuda()
        else:   # as the radius query pads them: short neighbourhoods repeat their first member
            nbr = ops.ball_query(radius, K, xyz, ops.index_points(xyz, centre))
            short = (nbr[..., 1:] == nbr[..., :1]).any(-1)
            assert bool(short.any()) and not bool(short.all())

    got = []
    tags = record(lambda: got.append(_sa_infer(level, xyz, pts, centre, nbr, K, ga, guard=GUARD, idx_out=idx_out)))
    new_xyz, out, (guard_xyz, guard_out) = got[0]

    kernel = "sa_infer_wide_kernel" if K > 32 else "sa_infer_kernel"
    tag = find(tags, f"{kernel} TM={c['tm']} G={B * S} K={K} D={D} C={ch[0]},{ch[1]},{ch[2]}")
    assert len(tag) == 1, (kernel, c["tm"], tags)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus == 256:
        assert field(tag[0], "split") == c["split"], tag[0]
    else:
        print(f"  {case}: {cus} CUs, not 256: the split= assertion is skipped ({tag[0]})")

    if search:   # the search the level ran itself, in the oracle's order
        oracle = request.getfixturevalue("oracle")
        want = oracle.knn_indices(oracle.index_points(xyz.cpu(), centre.cpu().long()), xyz.cpu(), K)
        assert torch.equal(idx_out.cpu().long(), want)
        assert find(tags, f"knn_kernel B={B} S={S} N={N} k={K}"), tags
        nbr = idx_out
    with torch.no_grad():   # the float64 evaluation of the same folded level, on the device
        ref, _ = _level64(xyz.double(), None if pts is None else pts.double(), None if ga else centre.long(), None if ga else nbr.long(),
                          _params64(level, "cuda"), False, fold=True)
    e = relmax(out, ref)
    print(f"  {case}: relmax {e:.3e} (gate {G2:.0e}); {tag[0]}")
    assert not torch.isnan(out).any() and not torch.isnan(new_xyz).any()
    if e > G2:   # which side is at fault: the library's float32 eval path on the same tensors
        with torch.no_grad():
            _, ev = ops.set_abstraction(xyz, pts, centre, K, ga, False, level.mlp_convs, level.mlp_bns, neighbour_idx=nbr)
        print(f"  {case}: eval path relmax {relmax(ev, ref):.3e}")
    assert e <= G2
    fill = torch.tensor(GUARD_FILL).view(torch.int32)
    assert bool((guard_out.view(torch.int32) == fill).all()) and bool((guard_xyz.view(torch.int32) == fill).all())
    if ga:
        assert torch.equal(new_xyz, torch.zeros_like(new_xyz))
    else:
        assert torch.equal(new_xyz, xyz[torch.arange(B, device="cuda")[:, None], centre.long()])
