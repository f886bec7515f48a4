"""GPU parity of every GEMM form the dispatcher selects by shape, each case proving which kernels it ran.

The set-abstraction levels do not run one kernel per product: a chain of shape predicates picks it (csrc/: wsf_applies, wsd3_applies,
wsx_applies / xyz0_applies, wsp_applies, wsq_applies, mid_gemm_shape_ok / mid_da_dw_plan, the bands of launch_gemm, kSmallM in
sa_api.hip).  Each case below puts one level through conftest.routed_level -- float64 with every ReLU and max-pool decision of the
HIP path injected, GATE = 1e-5 of each tensor's max-abs -- records the ProfScope tag of every launch (tests/dispatch.py), and asserts the
kernels its band must reach and the ones it must not.  Cases where the split / float32-MFMA product forms differ run in both, under the
same gate.  After every case the wave-pair kernels' bounded polls must not have given up.

  level (rows M)                  predicate crossed                                 kernels asserted (split form | mfma form where different)
  sa1 S128 K32 D0 [64,64,128], M = 4096 B
    B 1    M 4096                 M <= kSmallM, M < 8192: no wave-strip kernel       gemm_kernel<64,64> (layer 0, gathered), gemm_smallm
                                                                                      (layers 1-2 and their dA), dZ materialised (+dZ)
    B 2    M 8192                 xyz0 / wsf / wsd3 / wsx: M >= 8192 (first shape)   rel_moments, gemm_wsf03 | gemm_wsf0, gemm_wsf3<64> |
                                                                                      gemm_wsf<64,2>, gemm_wsd3<128,32,A5> | gemm_wsp,
                                                                                      gemm_wsx<64,1,S3> | gemm_wsx<64,1>, xyz0_post
    B 3    M 12288                inside the band                                    as B 2
    B 5    M 20480                640 strips > 4 x 128 wsd3 workers: ragged rounds    as B 2; gemm_wsd3 grid 256 (128 workers)
  sa1 S40 / S43, B 7 (custom)     workers = ceil(strips / 4) not a multiple of 8:     as B 2, with the plain worker map:
                                  no XCD map; S43: 301 strips, 76 workers, the last   gemm_wsf03 / wsx grid 70 | 76, gemm_wsf3 / wsd3 grid
                                  worker has one strip and three idle waves            140 | 152 (workers % 8 != 0 asserted);
                                  pooled epilogue needs M % 64 == 0 (gemm_pools_in_..) S40 pools in gemm_wsf3 (+pool), S43 in pool_fwd
  sa2 S32 K32 D128 [128,128,256], M = 1024 B, N 128 source points (layer 0 convolved before the gather)
    B 4    M 4096                 M <= kSmallM; mid tiles: layer 2 only (256 tiles)   gemm_smallm (layer 1), gemm_mid (layer 2, pooled
                                  mid_da_dw_plan: 136 tiles < 192                     in its epilogue), da_dw_kernel, +dZ
    B 5    M 5120                 kSmallM < M: no smallm, no da_dw; layer 1 has 160   gemm_kernel<64,64> (layer 1 fwd, dA of layers 1-2),
                                  mid tiles < 192                                     gemm_mid (layer 2 fwd)
    B 7    M 7168                 layer 1 reaches 224 mid tiles                       gemm_mid (layers 1-2 fwd), gemm_kernel<64,64> (dA)
    B 8    M 8192                 wsf / wsd3 / wsq: M >= 8192 (first shape)           gemm_wsf3<128> | gemm_wsf<128,2>, gemm_wsd3<256,32,A5>
                                                                                      | gemm_wsq, gemm_wsd3<128,32,A4> | gemm_ws<128,..,dW>
    B 9    M 9216                 288 strips: 36 wsf3 workers (plain map)            as B 8, gemm_wsf3 grids 72 / 144
    B 40   M 40960                1280 strips > 1024 wsf3 wave slots: ragged rounds  as B 8
  sa2 S43, B 7 (custom)           301 strips: wsf3 38 workers (plain map, last one    gemm_wsf3 grid 76 / 152 | gemm_wsf; gemm_wsd3 grid 256
                                  five strips); M % 64 = 32: no gemm_wsq               | gemm_ws<256,..,dW> (not gemm_wsq)
  sa3 group_all [256,512,1024], M = 32 B  (layer 0: 259 -> 256, layer 1: 256 -> 512, layer 2: 512 -> 1024)
    B 8    M 256                  M < 512: no mid tiles                               gemm_smallm everywhere, da_dw_kernel; pool_bwd fused away
    B 23   M 736                  M < 768 (layer 2: 12 x 16 mid tiles needed)         as B 8
    B 24   M 768                  first mid_gemm_shape_ok shape of layer 2            gemm_mid3 | gemm_mid (layer 2, +pool), da_dw_mid (dA 2)
    B 25   M 800                  M % 64 != 0                                         gemm_smallm (layer 2), da_dw_kernel, pool_fwd_kernel
    B 128  M 4096                 M == kSmallM; 64 groups < G: pool_bwd launch back  gemm_mid (layer 1), gemm_mid3 | gemm_mid (layer 2),
                                                                                      da_dw_mid (dA 1, 2), pool_bwd_kernel, +dZ
    B 129  M 4128                 kSmallM < M, M % 64 != 0                            gemm_kernel<64,64> (all products), dw_* launches
    B 256  M 8192                 last mid_gemm_shape_ok shape; try_launch_ws for     gemm_ws<256> (layer 1), gemm_mid3 | gemm_mid (layer 2,
                                  layer 1; pooled epilogue only below 8192 rows       pool_fwd_kernel), gemm_kernel<64,64> (dA)
    B 258  M 8256                 past mid_gemm_shape_ok's upper bound                gemm_ws<256> (layer 1), gemm_kernel<64,64> (layer 2)
    B 512  M 16384                M >= 128 x 128: tall tiles (layer 2 has K = 512:    gemm_kernel<128,128,4,2> (layers 0, 2, dA),
                                  no wave-strip form, no pooled epilogue)             gemm_ws<256> (layer 1), pool_fwd_kernel

gemm_wsd3<256> and <128,A4> always run with 64 workers (M >= 8192 gives at least 256 strips for 4 x 64 wave slots), so their XCD map
is the only one they can take; the custom shapes reach them with a ragged last round instead.  sa1 / sa2 change band again only at
B >= 2048 (the 32-bit offset guards), out of scope here.  Every case here runs with training=True; the same band edges in eval mode
(E_STORE products, BatchNorm from the running statistics) are tests/test_gpu_eval_bands.py.
"""
import pytest
import torch

from conftest import routed_level
from dispatch import expect, find, record, wave_strip_workers
from test_gpu_levels_routed import GATE

pytestmark = pytest.mark.gpu

SA1, SA2, SA3 = (128, 32, 0, [64, 64, 128], 1024), (32, 32, 128, [128, 128, 256], 128), (None, None, 256, [256, 512, 1024], 32)
BOTH, SPLIT = ("split", "mfma"), ("split",)

# the wave-strip kernels of a grouped level's large products, and the generic forms they replace
WS1_SPLIT = ["rel_moments_kernel", "gemm_wsf03_kernel", "gemm_wsf3_kernel<64", "gemm_wsd3_kernel<128,32,A5>", "gemm_wsx_kernel<64,1,S3>",
             "xyz0_post_kernel"]
WS1_MFMA = ["rel_moments_kernel", "gemm_wsf0_kernel", "gemm_wsf_kernel<64,2", "gemm_wsp_kernel", "gemm_wsx_kernel<64,1>", "xyz0_post_kernel"]
WS2_SPLIT = ["gather_rel_stats_kernel", "gemm_wsf3_kernel<128", "gemm_wsd3_kernel<256,32,A5>", "gemm_wsd3_kernel<128,32,A4>", "scatter_dz_kernel"]
WS2_MFMA = ["gather_rel_stats_kernel", "gemm_wsf_kernel<128,2", "gemm_wsq_kernel<256", "gemm_ws_kernel<128,64,64,A4,E2,dW>", "scatter_dz_kernel"]
WAVE_STRIP = ["gemm_wsf03", "gemm_wsf0_", "gemm_wsf3", "gemm_wsf_", "gemm_wsd3", "gemm_wsp", "gemm_wsq", "gemm_wsx", "rel_moments", "xyz0_post"]
MID = ["gemm_mid3_kernel", "gemm_mid_kernel", "da_dw_mid_kernel"]


def _ws(split, mfma):
    return {"split": (split, [t for t in mfma if t not in split]), "mfma": (mfma, [t for t in split if t not in mfma])}


def _same(present, absent=()):
    return {"split": (present, list(absent)), "mfma": (present, list(absent))}


def _sa3_l2(M, pooled):
    """layer 2 of sa3 on the 64 x 64 tiles: gemm_mid3 (split) or gemm_mid (mfma)"""
    p = " +pool" if pooled else ""
    return {"split": ([f"gemm_mid3_kernel M={M} N=1024"] + ([f"bn_finalize_fwd_kernel C=1024{p}"] if pooled else ["pool_fwd_kernel"]),
                      [f"gemm_mid_kernel M={M} N=1024"]),
            "mfma": ([f"gemm_mid_kernel M={M} N=1024"] + ([f"bn_finalize_fwd_kernel C=1024{p}"] if pooled else ["pool_fwd_kernel"]),
                     [f"gemm_mid3_kernel"])}


def _workers(n):
    """every wave-strip kernel of an sa1-shaped level with n persistent workers (1 or 2 column blocks)"""
    return {"split": [("gemm_wsf03_kernel", 1, n), ("gemm_wsf3_kernel<64", 2, n), ("gemm_wsd3_kernel<128", 2, n), ("gemm_wsx_kernel", 1, n)],
            "mfma": [("gemm_wsf0_kernel", 1, n), ("gemm_wsf_kernel<64", 2, n), ("gemm_wsp_kernel", 1, n), ("gemm_wsx_kernel", 1, n)]}


def _plus(exp, present=(), absent=()):
    return {m: (list(p) + list(present), list(a) + list(absent)) for m, (p, a) in exp.items()}


# case id -> (level, geometry (S, K, D, mlp, N), B, product forms, {form: (present, absent)}, wave-strip kernels whose worker count is
# checked: {form: [(pattern, column blocks, workers)]})
CASES = {
    "sa1-B1": ("sa1", SA1, 1, SPLIT, _same(["gemm_kernel<64,64,2,2,A2 M=4096", "gemm_smallm_kernel M=4096", "bn_finalize_bwd_kernel +dZ"],
                                           WAVE_STRIP), {}),
    "sa1-B2": ("sa1", SA1, 2, BOTH, _plus(_ws(WS1_SPLIT, WS1_MFMA), absent=["gemm_smallm", "gemm_kernel<", "bn_finalize_bwd_kernel +dZ",
                                                                      "gemm_ws_kernel"]), {}),
    "sa1-B3": ("sa1", SA1, 3, BOTH, _plus(_ws(WS1_SPLIT, WS1_MFMA), absent=["gemm_smallm", "gemm_kernel<", "gemm_ws_kernel"]), {}),
    "sa1-B5": ("sa1", SA1, 5, BOTH, _plus(_ws(WS1_SPLIT, WS1_MFMA), absent=["gemm_smallm", "gemm_kernel<", "gemm_ws_kernel"]),
               {"split": [("gemm_wsd3_kernel<128", 2, 128)]}),
    "sa1-S40-B7": ("sa1", (40, 32, 0, [64, 64, 128], 1024), 7, BOTH, _plus(_ws(WS1_SPLIT, WS1_MFMA), ["bn_finalize_fwd_kernel C=128 +pool"],
                                                                        ["gemm_ws_kernel", "pool_fwd_kernel"]),
                   _workers(70)),
    "sa1-S43-B7": ("sa1", (43, 32, 0, [64, 64, 128], 1024), 7, BOTH, _plus(_ws(WS1_SPLIT, WS1_MFMA), ["pool_fwd_kernel G=301"],
                                                                        ["gemm_ws_kernel", "bn_finalize_fwd_kernel +pool"]),
                   _workers(76)),
    "sa2-B4": ("sa2", SA2, 4, SPLIT, _same(["gemm_smallm_kernel M=4096 N=128", "gemm_mid_kernel M=4096 N=256", "bn_finalize_fwd_kernel C=256 +pool",
                                            "da_dw_kernel M=4096", "bn_finalize_bwd_kernel +dZ"], WAVE_STRIP + ["gemm_kernel<"]), {}),
    "sa2-B5": ("sa2", SA2, 5, SPLIT, _same(["gemm_kernel<64,64,2,2,A1,E1> M=5120 N=128", "gemm_mid_kernel M=5120 N=256",
                                            "gemm_kernel<64,64,2,2,A5,E2> M=5120", "gemm_kernel<64,64,2,2,A4,E2> M=5120"],
                                           WAVE_STRIP + ["gemm_smallm_kernel M=5120", "da_dw_kernel M=5120", "da_dw_mid", "bn_finalize_bwd_kernel +dZ"]), {}),
    "sa2-B7": ("sa2", SA2, 7, SPLIT, _same(["gemm_mid_kernel M=7168 N=128", "gemm_mid_kernel M=7168 N=256", "gemm_kernel<64,64,2,2,A5,E2> M=7168",
                                            "gemm_kernel<64,64,2,2,A4,E2> M=7168"], WAVE_STRIP + ["gemm_smallm_kernel M=7168", "da_dw_kernel M=7168", "da_dw_mid", "bn_finalize_bwd_kernel +dZ"]), {}),
    "sa2-B8": ("sa2", SA2, 8, BOTH, _plus(_ws(WS2_SPLIT, WS2_MFMA), absent=["gemm_smallm_kernel M=8192", "gemm_kernel< M=8192", "gemm_mid"]), {}),
    "sa2-B9": ("sa2", SA2, 9, BOTH, _plus(_ws(WS2_SPLIT, WS2_MFMA), absent=["gemm_kernel< M=9216", "gemm_mid"]),
               {"split": [("gemm_wsf3_kernel<128 M=9216 N=128", 2, 36), ("gemm_wsf3_kernel<128 M=9216 N=256", 4, 36)]}),
    "sa2-B40": ("sa2", SA2, 40, BOTH, _plus(_ws(WS2_SPLIT, WS2_MFMA), absent=["gemm_kernel< M=40960", "gemm_mid"]),
                {"split": [("gemm_wsf3_kernel<128 M=40960 N=128", 2, 128), ("gemm_wsd3_kernel<256", 4, 64)]}),
    "sa2-S43-B7": ("sa2", (43, 32, 128, [128, 128, 256], 128), 7, BOTH,
                   {"split": (["gemm_wsf3_kernel<128", "gemm_wsd3_kernel<256,32,A5>", "gemm_wsd3_kernel<128,32,A4>"], ["gemm_wsq", "gemm_wsf_"]),
                    "mfma": (["gemm_wsf_kernel<128,2", "gemm_ws_kernel<256,64,64,A5,E2,dW>", "gemm_ws_kernel<128,64,64,A4,E2,dW>"],
                             ["gemm_wsq", "gemm_wsf3", "gemm_wsd3"])},
                   {"split": [("gemm_wsf3_kernel<128 M=9632 N=128", 2, 38), ("gemm_wsf3_kernel<128 M=9632 N=256", 4, 38),
                              ("gemm_wsd3_kernel<256", 4, 64), ("gemm_wsd3_kernel<128", 4, 64)]}),
    "sa3-B8": ("sa3", SA3, 8, SPLIT, _same(["gemm_smallm_kernel M=256 N=1024", "gemm_smallm_kernel M=256 N=512", "da_dw_kernel M=256"],
                                           MID + ["gemm_kernel<", "pool_bwd_kernel", "gemm_ws"]), {}),
    "sa3-B23": ("sa3", SA3, 23, SPLIT, _same(["gemm_smallm_kernel M=736 N=1024", "da_dw_kernel M=736"], MID + ["gemm_kernel<", "pool_bwd_kernel"]), {}),
    "sa3-B24": ("sa3", SA3, 24, BOTH, _plus(_sa3_l2(768, True), ["gemm_smallm_kernel M=768 N=512", "da_dw_mid_kernel M=768"],
                                            ["gemm_kernel<", "pool_fwd_kernel", "pool_bwd_kernel"]), {}),
    "sa3-B25": ("sa3", SA3, 25, SPLIT, _same(["gemm_smallm_kernel M=800 N=1024", "da_dw_kernel M=800", "pool_fwd_kernel"], MID + ["gemm_kernel<"]), {}),
    "sa3-B128": ("sa3", SA3, 128, BOTH, _plus(_sa3_l2(4096, True), ["gemm_mid_kernel M=4096 N=512", "gemm_smallm_kernel M=4096 N=256",
                                                                     "da_dw_mid_kernel M=4096", "pool_bwd_kernel", "bn_finalize_bwd_kernel +dZ"],
                                              ["gemm_kernel<", "pool_fwd_kernel"]), {}),
    "sa3-B129": ("sa3", SA3, 129, SPLIT, _same(["gemm_kernel<64,64,2,2,A3,E1> M=4128", "gemm_kernel<64,64,2,2,A1,E1> M=4128 N=512",
                                                "gemm_kernel<64,64,2,2,A1,E1> M=4128 N=1024", "gemm_kernel<64,64,2,2,A5,E2> M=4128",
                                                "pool_fwd_kernel", "pool_bwd_kernel"], MID + ["gemm_smallm", "da_dw", "bn_finalize_bwd_kernel +dZ"]), {}),
    "sa3-B256": ("sa3", SA3, 256, BOTH, _plus(_sa3_l2(8192, False), ["gemm_ws_kernel<256,64,64,A1 M=8192", "gemm_kernel<64,64,2,2,A3,E1> M=8192",
                                                                     "gemm_kernel<64,64,2,2,A5,E2> M=8192"],
                                              ["gemm_smallm", "da_dw", "bn_finalize_fwd_kernel +pool"]), {}),
    "sa3-B258": ("sa3", SA3, 258, SPLIT, _same(["gemm_ws_kernel<256,64,64,A1 M=8256", "gemm_kernel<64,64,2,2,A1,E1> M=8256 N=1024",
                                                "pool_fwd_kernel"], MID + ["gemm_smallm", "da_dw"]), {}),
    "sa3-B512": ("sa3", SA3, 512, SPLIT, _same(["gemm_kernel<128,128,4,2,A3,E1> M=16384", "gemm_ws_kernel<256,64,64,A1 M=16384",
                                                "gemm_kernel<128,128,4,2,A1,E1> M=16384 N=1024", "gemm_kernel<128,128,4,2,A5,E2> M=16384",
                                                "pool_fwd_kernel"], MID + ["gemm_smallm", "da_dw", "gemm_kernel<64,64"]), {}),
}


@pytest.fixture()
def products():
    from pnpp_hip import ops
    before = ops.get_float32_products()
    yield ops
    ops.set_float32_products(before)


def _inputs(level, geo, B, seed):
    S, K, D, mlp, N = geo
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, N, 3, generator=g) * 2 - 1
    pts = torch.randn(B, N, D, generator=g) if D else None
    if level == "sa3":   # sa2's output: max-pooled ReLU activations
        pts = torch.randn(B, N, D, generator=g).abs()
    centres = None if S is None else torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)])
    gy = torch.randn(B, 1 if S is None else S, mlp[-1], generator=g)
    return xyz, pts, centres, gy


def _module(geo, seed):
    from models.pointnet_pp_8dir import PointNetSetAbstraction
    S, K, D, mlp, _ = geo
    torch.manual_seed(seed)
    sa = PointNetSetAbstraction(S, K, D, list(mlp), group_all=S is None)
    with torch.no_grad():
        for bn in sa.bns:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
    return sa.cuda().train()


PARAMS = [pytest.param(cid, form, id=f"{cid}-{form}") for cid, c in CASES.items() for form in c[3]]


@pytest.mark.parametrize("cid,form", PARAMS)
def test_band(oracle, products, cid, form):
    from pnpp_hip import _lib
    level, geo, B, _, exp, workers = CASES[cid]
    products.set_float32_products(form)
    seed = 1000 + B + 7 * (geo[0] or 0)
    sa = _module(geo, seed)
    xyz, pts, centres, gy = _inputs(level, geo, B, seed)
    out = {}
    tags = record(lambda: out.update(r=routed_level(oracle, sa, xyz, pts, centres, gy, geo[1], geo[0] is None, True)))
    res, diag = out["r"]
    torch.cuda.synchronize()
    print(f"\n[{cid} {form}] M={B * (geo[0] or 1) * (geo[1] or geo[4])} ReLU flips {diag['relu_flips']}; kernels:\n    " + "\n    ".join(tags) +
          "\n  error (rel-to-max): " + ", ".join(f"{k} {v:.2e}" for k, v in res.items()) + f"\n  worst {max(res.values()):.2e}")
    present, absent = exp[form]
    expect(tags, present, absent)
    for pattern, ncol, n in workers.get(form, []):
        hits = find(tags, pattern)
        assert hits, (pattern, tags)
        for t in hits:
            assert wave_strip_workers(t, ncol) == n, (t, n)
            if cid.startswith(("sa1-S", "sa2-S")) and ncol <= 2:
                assert n % 8 != 0, t   # the plain strip map ran: the XCD-aware one needs workers % 8 == 0
    assert _lib.lib().pnpp_debug_wsd3_timeouts() == 0
    assert max(res.values()) <= GATE, res
