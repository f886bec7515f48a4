"""GPU parity of the PointNet++ classifier's levels (models/pointnet_pp_cls.py) across the dispatcher's kernel bands, each case proving which
kernels it ran -- tests/test_gpu_dispatch_bands.py for the three geometries only the classifier has:

  level 1      D = 3, K = 32, [64,64,128]: a level WITH features whose width is no multiple of 4.  xyz0_applies / wsx_applies need D == 0,
               sa_level_plan's `delayed` needs D % 4 == 0, try_launch_ws gathers only D == 0 or D == 128: layer 0 always runs the chunked
               gemm_kernel through fetch_a4's scalar branch, layer 1's backward the generic weights-stationary dA + dW form.  The model
               detaches the normals; asked for, the level returns their gradient too (dF = dZ_0 W_f with N = 3 on the generic GEMM, then
               scatter_rows_bwd C=3): sa_backward used to refuse any D % 4 != 0 there, which only the whole-cloud level's paired
               dA + dW launch needs (csrc/sa_api.hip: sa_level_bwd).
  level 2     D = 128, K = 64, [128,128,256]: every predicate gated on 32 neighbours is false (wsq_applies, wsp_applies and the pooled
               branch of wsd3_applies test A.K, gemm_pools_in_epilogue tests nsample), so the last layer's backward is
               gemm_ws_kernel<256,..,A5,E2,dW> on the general rc / K, row % K path and the pooling a pool_fwd_kernel over 64 rows.
  whole cloud  128 rows per cloud, [256,512,1024]: M = 128 B crosses kSmallM, mid_gemm_shape_ok and mid_da_dw_plan at other batch sizes
               than the 32-row sa3, and nsample = 128 rules the pooled epilogue out everywhere.

Neighbourhoods come from ops.ball_query: every grouped case asserts, before the level runs, that some are full and some padded (a short
neighbourhood repeats its first member: exact arg-max ties, duplicated rows in the BatchNorm sums and in scatter_dz); the "padded" cases
build a tight cluster of K + 8 points (always a full neighbourhood), a sparse remainder and one far-away point forced to be a centre -- K
copies of one point.

Each case runs ops.set_abstraction forward + backward once with ops.sa_tap armed, under dispatch.record, and evaluates
oracle.sa_forward in float64 on the same indices with the tapped arg-max and ReLU decisions injected.  Asserted, as conftest.routed_level
does: route_gap <= ROUTE_GAP, relu_flip_margin <= FLIP_MARGIN, train-mode conv-bias gradients exactly zero, the structurally-zero rule,
running statistics against BNState.updates (eval: untouched); every returned tensor (out, d_points, d_<param>, rm_l, rv_l) within GATE =
1e-5 of its max-abs; the tags; pnpp_debug_wsd3_timeouts() == 0.  BatchNorm affine parameters AND running statistics are moved off their
defaults.  Cases whose kernels differ between the split / float32-MFMA product forms run in both.

The present / absent lists are derived from the predicates in csrc/ (named per row), not from a run; the first run on the MI355X agreed
with every one of them.  Two places where the
code says something else than "no +pool tag anywhere" for these levels:
  * "+pool" on bn_finalize_FWD is the pooled GEMM epilogue: absent in every level-2 and whole-cloud case (nsample != 32).  Level 1 has
    K = 32 and does pool in gemm_wsf3 / gemm_wsf where gemm_pools_in_epilogue holds (train, M >= 8192, M % 64 == 0): asserted present.
  * "+pool" on bn_finalize_BWD is sa_bwd_top's pooled source (the finalisation takes dout itself, no pool_bwd launch): it needs
    M <= kSmallM and G <= 64 and does not look at K, so l2-small (G = 64) and ga-B3 / B6 / B32 take it: asserted present there, absent
    (and pool_bwd_kernel present) everywhere else.

  case (rows M)                  predicate crossed                                   kernels asserted present (split | mfma) ; absent         worst error (split | mfma)
  level 1: S x 32 rows per cloud, N = 256, radius 0.65 (padded: 0.4)
    l1-small   B2 S64   4096     sa_api.hip kSmallM: M <= 4096; launch_gemm: M < 8192  gemm_kernel<64,64,2,2,A2,E1> (layer 0), gemm_smallm     4.8e-7
                                                                                       N=64 / 128 / 3 (dF), +dZ, pool_fwd, pool_bwd ; every
                                                                                       wave-strip kernel, gemm_ws, da_dw (K' = 64 < 128)
    l1-first   B2 S128  8192     wsf_applies, wsd3_applies (pooled, K == 32, 128->64)  gemm_kernel<..,A2,E1>, gemm_wsf3<64> N=64, N=128 |      5.2e-7 | 5.4e-7
                                 | wsp_applies; try_launch_ws Kd == 64 for layer 1's    gemm_wsf<64,2>, gemm_wsd3<128,32,A5> | gemm_wsp,
                                 dA + dW; gemm_pools_in_epilogue (K = 32, M % 64 == 0)  gemm_ws<64,64,64,A4,E2,dW>, dw_kernel<A4,A2>,
                                                                                       gemm_kernel<128,32,4,1,A4,E0> N=3 (dF), scatter_rows_bwd
                                                                                       C=3, bn_finalize_fwd C=128 +pool ; gemm_wsx, xyz0_post,
                                                                                       rel_moments, gemm_wsf03, gemm_wsf0, gather_rel_stats,
                                                                                       scatter_dz, gemm_wsq, gemm_smallm, pool_fwd
    l1-ragged  B7 S43   9632     301 strips, 76 workers (% 8 != 0: plain strip map);    as l1-first with grids 76 (N=64), 152 (N=128, wsd3),    8.7e-7 | 7.8e-7
                                 M % 64 = 32: gemm_pools_in_epilogue false              76 (wsp) and pool_fwd_kernel ; bn_finalize_fwd +pool
    l1-padded  l1-first, cluster + far centre, radius 0.4                               as l1-first                                             1.4e-6 | 1.2e-6
    l1-eval    l1-first, training=False: E_STORE forward, sa_forward_impl pools         gemm_kernel<..,A2,E0>, gemm_wsf3<64,A1,E0> |            2.7e-7 | 2.8e-7
               in pool_fwd (the pooled epilogue is train-only)                          gemm_wsf<64,2,A1,E0>, backward as l1-first, pool_fwd
  level 2: S x 64 rows per cloud, N = 128, radius 1.1 (padded: 0.5); layer 0 convolved before the gather where S K > N
    l2-small   B2 S32   4096     kSmallM; mid_gemm_shape_ok: layer 2 only (256 tiles);  gather_rel_stats, gemm_smallm N=128, gemm_mid N=256,     1.9e-6
                                 mid_da_dw_plan 136 tiles < 192; sa_bwd_top G = 64      pool_fwd K=64, da_dw_kernel M=4096, bn_finalize_bwd
                                                                                       +dZ +pool, scatter_dz ; wave-strip, gemm_kernel<, gemm_ws,
                                                                                       pool_bwd
    l2-mid     B2 S40   5120     kSmallM < M < 8192; layer 1 has 160 mid tiles < 192    gemm_kernel<64,64,2,2,A1,E1> N=128, gemm_mid N=256,      1.0e-6
                                                                                       gemm_kernel<..,A5,E2>, <..,A4,E2>, dw_kernel, pool_fwd,
                                                                                       pool_bwd ; wave-strip, gemm_ws, gemm_smallm M=5120,
                                                                                       da_dw M=5120, +dZ
    l2-first   B2 S64   8192     wsf_applies; wsd3_applies dense (128->128) |           gather_rel_stats, gemm_wsf3<128> N=128, N=256 |          1.7e-6 | 1.8e-6
                                 try_launch_ws Kd == 128; last layer: wsd3 pooled,      gemm_wsf<128,2>, gemm_wsd3<128,32,A4> | gemm_ws<128,64,
                                 wsp, wsq all need A.K == 32 -> try_launch_ws Kd == 256 64,A4,E2,dW>, gemm_ws<256,64,64,A5,E2,dW>, pool_fwd K=64,
                                                                                       pool_bwd K=64, scatter_dz, da_dw_kernel<E0,A0> (dF + dW_f)
                                                                                       ; gemm_wsq, gemm_wsp, gemm_wsd3<256, gemm_wsd3<128,32,A5>,
                                                                                       any +pool, gemm_kernel<, gemm_mid, gemm_smallm M=8192
    l2-ragged  B3 S43   8256     258 strips: wsf3 33 workers (last has two strips),     as l2-first, gemm_wsf3 grids 66 / 132, gemm_wsd3<128,32,  1.3e-6 | 1.2e-6
                                 wsd3 64 workers x 4 waves + 2 strips in a second round A4> grid 256
    l2-padded  l2-first, cluster + far centre (64 copies of one point), radius 0.5      as l2-first                                             1.3e-6 | 1.2e-6
    l2-eval    l2-first, training=False                                                 as l2-first with E0 forward products                    2.3e-7 | 2.8e-7
    l2-gathered B64 S2  8192     sa_level_plan: S K = N, layer 0 not delayed;           gemm_ws<132,64,64,A2,E1> (layer 0), dw_kernel<A4,A2>,     6.9e-7 | 7.4e-7
                                 try_launch_ws gather form D == 128                     gemm_ws<128,64,64,A4,E0> + scatter_rows_bwd C=128 (dF),
                                                                                       layers 1-2 as l2-first ; gather_rel_stats, scatter_dz,
                                                                                       da_dw, gemm_kernel<
  whole cloud: 128 rows per cloud, points |randn|; pool_fwd_kernel K=128 present and bn_finalize_fwd +pool absent in every case
    ga-B3      384               mid_gemm_shape_ok / mid_da_dw_plan: M < 512            gemm_smallm N=256 / 512 / 1024, da_dw_kernel M=384,       5.9e-7
                                                                                       bn_finalize_bwd +dZ +pool ; gemm_mid*, da_dw_mid,
                                                                                       gemm_kernel<, gemm_ws, pool_bwd
    ga-B6      768               first mid shape of layer 2 (12 x 16 tiles); layer 2's  gemm_mid3 | gemm_mid N=1024, gemm_smallm N=512,           1.0e-6 | 8.5e-7
                                 dA + dW on mid tiles (12 x 8 + 128), layer 1's not     da_dw_mid M=768, da_dw_kernel M=768, +dZ +pool ;
                                 (12 x 4 + 32 < 192)                                    gemm_kernel<, pool_bwd
    ga-B32     4096              M == kSmallM; G = 32 <= 64: pooled source (the 32-row  gemm_smallm N=256, gemm_mid N=512, gemm_mid3 | gemm_mid     1.2e-6 | 1.3e-6
                                 sa3 has G = 128 here and launches pool_bwd)            N=1024, da_dw_mid M=4096, da_dw_kernel<E0,A3> (layer 0),
                                                                                       +dZ +pool ; gemm_kernel<, pool_bwd
    ga-B33     4224              past kSmallM, still M % 64 == 0: mid tiles forward,    gemm_kernel<64,64,2,2,A3,E1>, gemm_mid N=512, gemm_mid3 |   1.2e-6 | 1.1e-6
                                 generic backward                                       gemm_mid N=1024, gemm_kernel<..,A5,E2>, <..,A4,E2>,
                                                                                       pool_bwd ; gemm_smallm, da_dw, +dZ, bwd +pool
    ga-B64     8192              last mid_gemm_shape_ok shape; try_launch_ws (Kd = 256) gemm_ws<256,64,64,A1 (layer 1), gemm_mid3 | gemm_mid         1.2e-6 | 1.2e-6
                                 for layer 1 and for dF                                 N=1024, gemm_kernel<..,A3,E1>, <..,A5,E2>,
                                                                                       gemm_ws<256,64,64,A4,E0> (dF) ; gemm_smallm, da_dw
    ga-B65     8320              past mid_gemm_shape_ok                                 gemm_ws<256,64,64,A1, gemm_kernel<64,64,2,2,A1,E1> N=1024    1.3e-6
                                                                                       ; gemm_mid*, gemm_smallm, da_dw
    ga-B128    16384             launch_gemm: M >= 128 x 128, tall tiles                gemm_kernel<128,128,4,2,A3,E1>, <..,A1,E1> N=1024,           1.3e-6
                                                                                       <..,A5,E2>, gemm_ws<256,64,64,A1 ; gemm_mid*,
                                                                                       gemm_smallm, da_dw, gemm_kernel<64,64

Measured on the MI355X (rel-to-max, worst tensor of the case): level 1 2.7e-7 ... 1.4e-6, level 2 2.3e-7 ... 1.9e-6, whole cloud
5.9e-7 ... 1.3e-6, the two product forms alike; no injected decision further than 1.8e-7 (ReLU) / 4.8e-7 (arg-max) from float64's own.
"""
import pytest
import torch

from conftest import FLIP_MARGIN, ROUTE_GAP, relmax, tap_to_routing
from dispatch import expect, find, record, wave_strip_workers
from test_gpu_levels_routed import GATE

pytestmark = pytest.mark.gpu

BOTH, SPLIT = ("split", "mfma"), ("split",)
# family -> (K, D, mlp, N, radius, radius of the padded construction)
FAMILY = {"l1": (32, 3, [64, 64, 128], 256, 0.65, 0.4), "l2": (64, 128, [128, 128, 256], 128, 1.1, 0.5),
          "ga": (128, 256, [256, 512, 1024], 128, None, None)}

WAVE_STRIP = ["gemm_wsf03", "gemm_wsf0_", "gemm_wsf3", "gemm_wsf_", "gemm_wsd3", "gemm_wsp", "gemm_wsq", "gemm_wsx", "rel_moments", "xyz0_post"]
MID = ["gemm_mid3_kernel", "gemm_mid_kernel", "da_dw_mid_kernel"]
FWD_POOL, BWD_POOL = "bn_finalize_fwd_kernel +pool", "bn_finalize_bwd_kernel +pool"
# a level with features never takes the coordinate-level shortcut; one whose width is no multiple of 4 is never convolved before the gather
L1_NEVER = ["gemm_wsx", "xyz0_post", "rel_moments", "gemm_wsf03", "gemm_wsf0_", "gather_rel_stats", "scatter_dz", "gemm_wsq", "gemm_mid", "da_dw"]
# the kernels gated on 32 neighbours, and the pooled GEMM epilogue
L2_NEVER = ["gemm_wsq", "gemm_wsp", "gemm_wsd3_kernel<256", "gemm_wsd3_kernel<128,32,A5>", FWD_POOL, "gemm_wsx", "xyz0_post", "rel_moments",
            "gemm_wsf03", "gemm_wsf0_"]


def _forms(split, mfma, present=(), absent=()):
    """{form: (present, absent)}: the form's own kernels, the other form's kernels among the absent ones"""
    return {"split": (list(split) + list(present), [t.split()[0] for t in mfma if t not in split] + list(absent)),
            "mfma": (list(mfma) + list(present), [t.split()[0] for t in split if t not in mfma] + list(absent))}


def _same(present, absent=()):
    return {"split": (list(present), list(absent)), "mfma": (list(present), list(absent))}


def _l1(fwd_e, pooled):
    """level 1 at M >= 8192: fwd_e = 1 (train: E_STORE_STATS) or 0 (eval: E_STORE)"""
    split = [f"gemm_wsf3_kernel<64,A1,E{fwd_e}> N=64", f"gemm_wsf3_kernel<64,A1,E{fwd_e}> N=128", "gemm_wsd3_kernel<128,32,A5>"]
    mfma = [f"gemm_wsf_kernel<64,2,A1,E{fwd_e}> N=64", f"gemm_wsf_kernel<64,2,A1,E{fwd_e}> N=128", "gemm_wsp_kernel"]
    present = [f"gemm_kernel<64,64,2,2,A2,E{fwd_e}> N=64 K=8", "gemm_ws_kernel<64,64,64,A4,E2,dW>", "dw_kernel<A4,A2>", "pool_bwd_kernel K=32",
               "gemm_kernel<128,32,4,1,A4,E0> N=3", "scatter_rows_bwd_kernel C=3"]
    pool = (["bn_finalize_fwd_kernel C=128 +pool"], ["pool_fwd_kernel"]) if pooled else (["pool_fwd_kernel K=32"], [FWD_POOL])
    return _forms(split, mfma, present + pool[0], L1_NEVER + ["gemm_smallm", BWD_POOL, "bn_finalize_bwd_kernel +dZ"] + pool[1])


def _l2(fwd_e, M, gathered=False):
    """level 2 at M >= 8192"""
    split = [f"gemm_wsf3_kernel<128,A1,E{fwd_e}> N=128", f"gemm_wsf3_kernel<128,A1,E{fwd_e}> N=256", "gemm_wsd3_kernel<128,32,A4>"]
    mfma = [f"gemm_wsf_kernel<128,2,A1,E{fwd_e}> N=128", f"gemm_wsf_kernel<128,2,A1,E{fwd_e}> N=256", "gemm_ws_kernel<128,64,64,A4,E2,dW>"]
    present = ["gemm_ws_kernel<256,64,64,A5,E2,dW>", "pool_fwd_kernel K=64", "pool_bwd_kernel K=64"]
    absent = L2_NEVER + [f"gemm_smallm_kernel M={M}", "gemm_kernel<", "gemm_mid", BWD_POOL, "bn_finalize_bwd_kernel +dZ"]
    if gathered:
        present += [f"gemm_ws_kernel<132,64,64,A2,E{fwd_e}>", "dw_kernel<A4,A2>", "gemm_ws_kernel<128,64,64,A4,E0>", "scatter_rows_bwd_kernel C=128"]
        absent += ["gather_rel_stats", "scatter_dz", "da_dw"]
    else:
        present += ["gather_rel_stats_kernel", "scatter_dz_kernel", "da_dw_kernel<E0,A0>"]
    return _forms(split, mfma, present, absent)


def _ga(M, l2_mid, present=(), absent=()):
    """whole-cloud level: pool_fwd_kernel always, never the pooled epilogue; layer 2 on gemm_mid3 (split) / gemm_mid (mfma) where l2_mid"""
    present, absent = ["pool_fwd_kernel K=128"] + list(present), [FWD_POOL, "pool_fwd_split", "gemm_wsf", "gemm_wsd3", "gemm_wsp", "gemm_wsq", "gemm_wsx"] + list(absent)
    if not l2_mid:
        return _same(present, absent)
    return {"split": (present + [f"gemm_mid3_kernel M={M} N=1024"], absent + [f"gemm_mid_kernel M={M} N=1024"]),
            "mfma": (present + [f"gemm_mid_kernel M={M} N=1024"], absent + ["gemm_mid3_kernel"])}


# case id -> (family, B, S, training, padded, product forms, {form: (present, absent)}, {form: [(pattern, column blocks, workers)]})
CASES = {
    "l1-small": ("l1", 2, 64, True, False, SPLIT,
                 _same(["gemm_kernel<64,64,2,2,A2,E1> M=4096 K=8", "gemm_smallm_kernel M=4096 N=64", "gemm_smallm_kernel M=4096 N=128",
                        "gemm_smallm_kernel M=4096 N=3", "scatter_rows_bwd_kernel C=3", "bn_finalize_bwd_kernel +dZ", "pool_fwd_kernel K=32",
                        "pool_bwd_kernel K=32"], WAVE_STRIP + L1_NEVER + ["gemm_ws_kernel", FWD_POOL, BWD_POOL]), {}),
    "l1-first": ("l1", 2, 128, True, False, BOTH, _l1(1, True), {}),
    "l1-ragged": ("l1", 7, 43, True, False, BOTH, _l1(1, False),
                  {"split": [("gemm_wsf3_kernel<64 M=9632 N=64", 1, 76), ("gemm_wsf3_kernel<64 M=9632 N=128", 2, 76), ("gemm_wsd3_kernel<128", 2, 76)],
                   "mfma": [("gemm_wsf_kernel<64 M=9632 N=64", 1, 76), ("gemm_wsf_kernel<64 M=9632 N=128", 2, 76), ("gemm_wsp_kernel", 1, 76)]}),
    "l1-padded": ("l1", 2, 128, True, True, BOTH, _l1(1, True), {}),
    "l1-eval": ("l1", 2, 128, False, False, BOTH, _l1(0, False), {}),
    "l2-small": ("l2", 2, 32, True, False, SPLIT,
                 _same(["gather_rel_stats_kernel", "gemm_smallm_kernel M=4096 N=128", "gemm_mid_kernel M=4096 N=256", "pool_fwd_kernel K=64",
                        "da_dw_kernel M=4096", "bn_finalize_bwd_kernel +dZ +pool", "scatter_dz_kernel"],
                       WAVE_STRIP + L2_NEVER + ["gemm_kernel<", "gemm_ws_kernel", "pool_bwd_kernel", "gemm_mid3"]), {}),
    "l2-mid": ("l2", 2, 40, True, False, SPLIT,
               _same(["gather_rel_stats_kernel", "gemm_kernel<64,64,2,2,A1,E1> M=5120 N=128", "gemm_mid_kernel M=5120 N=256", "pool_fwd_kernel K=64",
                      "pool_bwd_kernel K=64", "gemm_kernel<64,64,2,2,A5,E2> M=5120", "gemm_kernel<64,64,2,2,A4,E2> M=5120", "dw_kernel<A5,A1>",
                      "dw_kernel<A4,A1>", "scatter_dz_kernel"],
                     WAVE_STRIP + L2_NEVER + ["gemm_ws_kernel", "gemm_smallm_kernel M=5120", "da_dw_kernel M=5120", "da_dw_mid", BWD_POOL,
                                              "bn_finalize_bwd_kernel +dZ", "gemm_mid3"]), {}),
    "l2-first": ("l2", 2, 64, True, False, BOTH, _l2(1, 8192), {}),
    "l2-ragged": ("l2", 3, 43, True, False, BOTH, _l2(1, 8256),
                  {"split": [("gemm_wsf3_kernel<128 M=8256 N=128", 2, 33), ("gemm_wsf3_kernel<128 M=8256 N=256", 4, 33), ("gemm_wsd3_kernel<128", 4, 64)]}),
    "l2-padded": ("l2", 2, 64, True, True, BOTH, _l2(1, 8192), {}),
    "l2-eval": ("l2", 2, 64, False, False, BOTH, _l2(0, 8192), {}),
    "l2-gathered": ("l2", 64, 2, True, False, BOTH, _l2(1, 8192, gathered=True), {}),
    "ga-B3": ("ga", 3, None, True, False, SPLIT,
              _ga(384, False, ["gemm_smallm_kernel M=384 N=256", "gemm_smallm_kernel M=384 N=512", "gemm_smallm_kernel M=384 N=1024", "da_dw_kernel M=384",
                               "bn_finalize_bwd_kernel +dZ +pool"], MID + ["gemm_kernel<", "gemm_ws_kernel", "pool_bwd_kernel"]), {}),
    "ga-B6": ("ga", 6, None, True, False, BOTH,
              _ga(768, True, ["gemm_smallm_kernel M=768 N=256", "gemm_smallm_kernel M=768 N=512", "da_dw_mid_kernel M=768", "da_dw_kernel M=768",
                              "bn_finalize_bwd_kernel +dZ +pool"], ["gemm_kernel<", "gemm_ws_kernel", "pool_bwd_kernel"]), {}),
    "ga-B32": ("ga", 32, None, True, False, BOTH,
               _ga(4096, True, ["gemm_smallm_kernel M=4096 N=256", "gemm_mid_kernel M=4096 N=512", "da_dw_mid_kernel M=4096", "da_dw_kernel<E0,A3> M=4096",
                                "bn_finalize_bwd_kernel +dZ +pool"], ["gemm_kernel<", "gemm_ws_kernel", "pool_bwd_kernel"]), {}),
    "ga-B33": ("ga", 33, None, True, False, BOTH,
               _ga(4224, True, ["gemm_kernel<64,64,2,2,A3,E1> M=4224", "gemm_mid_kernel M=4224 N=512", "gemm_kernel<64,64,2,2,A5,E2> M=4224",
                                "gemm_kernel<64,64,2,2,A4,E2> M=4224", "gemm_kernel<64,64,2,2,A4,E0> M=4224", "pool_bwd_kernel K=128"],
                   ["gemm_smallm", "da_dw", "bn_finalize_bwd_kernel +dZ", BWD_POOL, "gemm_ws_kernel"]), {}),
    "ga-B64": ("ga", 64, None, True, False, BOTH,
               _ga(8192, True, ["gemm_kernel<64,64,2,2,A3,E1> M=8192", "gemm_ws_kernel<256,64,64,A1,E1> M=8192", "gemm_kernel<64,64,2,2,A5,E2> M=8192",
                                "gemm_kernel<64,64,2,2,A4,E2> M=8192", "gemm_ws_kernel<256,64,64,A4,E0> M=8192", "pool_bwd_kernel K=128"],
                   ["gemm_smallm", "da_dw", "bn_finalize_bwd_kernel +dZ", BWD_POOL, "gemm_mid_kernel M=8192 N=512"]), {}),
    "ga-B65": ("ga", 65, None, True, False, SPLIT,
               _ga(8320, False, ["gemm_kernel<64,64,2,2,A3,E1> M=8320", "gemm_ws_kernel<256,64,64,A1,E1> M=8320", "gemm_kernel<64,64,2,2,A1,E1> M=8320 N=1024",
                                 "gemm_kernel<64,64,2,2,A5,E2> M=8320", "gemm_ws_kernel<256,64,64,A4,E0> M=8320", "pool_bwd_kernel K=128"],
                   MID + ["gemm_smallm", "da_dw", BWD_POOL]), {}),
    "ga-B128": ("ga", 128, None, True, False, SPLIT,
                _ga(16384, False, ["gemm_kernel<128,128,4,2,A3,E1> M=16384", "gemm_ws_kernel<256,64,64,A1,E1> M=16384",
                                   "gemm_kernel<128,128,4,2,A1,E1> M=16384 N=1024", "gemm_kernel<128,128,4,2,A5,E2> M=16384",
                                   "gemm_kernel<128,128,4,2,A4,E2> M=16384", "pool_bwd_kernel K=128"],
                    MID + ["gemm_smallm", "da_dw", "gemm_kernel<64,64", BWD_POOL]), {}),
}


@pytest.fixture()
def products():
    from pnpp_hip import ops
    before = ops.get_float32_products()
    yield ops
    ops.set_float32_products(before)


def _inputs(cid):
    """-> xyz (B,N,3), pts (B,N,D), centres (B,S) or None, gy (B,S or 1,C), radius or None; the same for both product forms of a case"""
    fam, B, S, _, padded, _, _, _ = CASES[cid]
    K, D, mlp, N, radius, radius_padded = FAMILY[fam]
    g = torch.Generator().manual_seed(3000 + 97 * list(CASES).index(cid))
    xyz = torch.rand(B, N, 3, generator=g) * 2 - 1
    pts = torch.randn(B, N, D, generator=g)
    if fam == "ga":   # level 2's output: max-pooled ReLU activations
        return xyz, pts.abs(), None, torch.randn(B, 1, mlp[-1], generator=g), None
    if not padded:
        centres = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)])
    else:
        # K + 8 points in a cube of side radius / 2 (any two closer than 0.87 radius: every one of them has a full neighbourhood), the
        # uniform remainder (sparse against this radius), and a last point nothing else is near; centres: that point, a cluster point,
        # then a random prefix of the others
        radius = radius_padded
        xyz[:, :K + 8] = torch.tensor([0.3, -0.2, 0.1]) + (torch.rand(B, K + 8, 3, generator=g) * 2 - 1) * radius / 4
        xyz[:, N - 1] = 4.0
        centres = torch.stack([torch.cat([torch.tensor([N - 1, 0]), 1 + torch.randperm(N - 2, generator=g)[:S - 2]]) for _ in range(B)])
    return xyz, pts, centres, torch.randn(B, S, mlp[-1], generator=g), radius


def _members(nbr):
    """members of each neighbourhood as the radius query pads it: a short one repeats its first member to the end"""
    return 1 + (nbr[..., 1:] != nbr[..., :1]).sum(-1)


def _level(cid):
    from models.pointnet_pp_cls import SimpleSetAbstraction, SimpleSetAbstractionGroupAll
    fam, B, S, training, _, _, _, _ = CASES[cid]
    K, D, mlp, N, radius, _ = FAMILY[fam]
    torch.manual_seed(4000 + list(CASES).index(cid))
    level = SimpleSetAbstractionGroupAll(D, list(mlp)) if fam == "ga" else SimpleSetAbstraction(S, radius, K, D, list(mlp))
    with torch.no_grad():
        for bn in level.mlp_bns:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
            bn.running_mean.normal_(0.0, 0.3)
            bn.running_var.uniform_(0.5, 2.0)
    return level.cuda().train(training)


def _routed(oracle, level, xyz, pts, centres, nbr, gy, K, group_all, training):
    """conftest.routed_level for a level that is handed its indices: ops.set_abstraction(..., neighbour_idx=) forward + backward against
    oracle.sa_forward in float64 with the tapped arg-max and ReLU decisions.  -> ({tensor: rel-to-max error}, diag, [what else is wrong])"""
    from pnpp_hip import ops
    level.zero_grad()
    P, wrong = {}, []
    for l, (conv, bn) in enumerate(zip(level.mlp_convs, level.mlp_bns)):   # before the HIP forward pass updates the running statistics
        for name, t in ((f"convs.{l}.weight", conv.weight), (f"convs.{l}.bias", conv.bias), (f"bns.{l}.weight", bn.weight), (f"bns.{l}.bias", bn.bias)):
            P["sa." + name] = t.detach().cpu().double().requires_grad_(True)
        P[f"sa.bns.{l}.running_mean"], P[f"sa.bns.{l}.running_var"] = bn.running_mean.detach().cpu().double(), bn.running_var.detach().cpu().double()
    before = [(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)) for bn in level.mlp_bns]
    pts_gpu = pts.cuda().requires_grad_(True)
    ops.sa_tap = []
    try:
        _, y = ops.set_abstraction(xyz.cuda(), pts_gpu, None if group_all else centres.to(torch.int32).cuda(), None if group_all else K, group_all,
                                   training, level.mlp_convs, level.mlp_bns, neighbour_idx=nbr)
        routing = tap_to_routing(ops.sa_tap)[0]
    finally:
        ops.sa_tap = None
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    if not group_all:
        assert torch.equal(routing["neighbours"], nbr.cpu().long())
    pts64 = pts.double().requires_grad_(True)
    diag, st = {}, oracle.BNState()
    _, y64, _ = oracle.sa_forward(xyz, pts64, P, "sa", centres, None if group_all else K, group_all, training, st,
                                  neighbour_idx=routing["neighbours"], argmax=routing["argmax"], relu_masks=routing["relu_masks"], diag=diag)
    (y64 * gy.double()).sum().backward()
    if max(diag["route_gap"]) > ROUTE_GAP:
        wrong.append(f"route_gap {diag['route_gap']}")
    if max(diag["relu_flip_margin"]) > FLIP_MARGIN:
        wrong.append(f"relu_flip_margin {diag['relu_flip_margin']} ({diag['relu_flips']} flips)")
    res = {"out": relmax(y, y64), "d_points": relmax(pts_gpu.grad, pts64.grad)}
    for name, p in level.named_parameters():
        key = name.replace("mlp_", "")
        ref = P["sa." + key].grad
        if training and key.startswith("convs") and key.endswith("bias"):   # cancels in train-mode BatchNorm
            if not (float(p.grad.abs().max()) == 0.0 and float(ref.abs().max()) < 1e-9):
                wrong.append(f"{key}: gradient not zero ({float(p.grad.abs().max()):.1e}, float64 {float(ref.abs().max()):.1e})")
            continue
        if float(ref.abs().max()) < 1e-9:   # structurally zero: float32 can only produce noise here
            if not float(p.grad.abs().max()) < 1e-3:
                wrong.append(f"{key}: structurally zero, got {float(p.grad.abs().max()):.1e}")
            continue
        res["d_" + key] = relmax(p.grad, ref)
    for l, (bn, (rm, rv, nbt)) in enumerate(zip(level.mlp_bns, before)):
        if training:
            rm64, rv64 = st.updates[f"sa.bns.{l}"]
            res[f"rm_{l}"], res[f"rv_{l}"] = relmax(bn.running_mean, rm64), relmax(bn.running_var, rv64)
            if int(bn.num_batches_tracked) != nbt + 1:
                wrong.append(f"bns.{l}.num_batches_tracked {int(bn.num_batches_tracked)}")
        elif not (torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv) and int(bn.num_batches_tracked) == nbt):
            wrong.append(f"bns.{l}: an eval-mode pass wrote to the running statistics")
    return res, diag, wrong


PARAMS = [pytest.param(cid, form, id=f"{cid}-{form}") for cid, c in CASES.items() for form in c[5]]


@pytest.mark.parametrize("cid,form", PARAMS)
def test_band(oracle, products, cid, form):
    from pnpp_hip import _lib
    fam, B, S, training, padded, _, exp, workers = CASES[cid]
    K, D, mlp, N, _, _ = FAMILY[fam]
    group_all = fam == "ga"
    products.set_float32_products(form)
    level = _level(cid)
    xyz, pts, centres, gy, radius = _inputs(cid)
    nbr = None
    if not group_all:
        xg = xyz.cuda()
        nbr = products.ball_query(radius, K, xg, products.index_points(xg, centres.cuda()))
        n = _members(nbr.cpu())
        assert bool((n == K).any()) and bool((n < K).any()), "the radius must leave full and padded neighbourhoods"
        if padded:
            assert bool((n[:, 0] == 1).all()) and bool((n[:, 1] == K).all()), "the far centre is alone, the cluster centre's neighbourhood is full"
    out = {}
    tags = record(lambda: out.update(r=_routed(oracle, level, xyz, pts, centres, nbr, gy, K, group_all, training)))
    res, diag, wrong = out["r"]
    torch.cuda.synchronize()
    M = B * (N if group_all else S * K)
    print(f"\n[{cid} {form}] M={M} ReLU flips {diag['relu_flips']} (margin {max(diag['relu_flip_margin']):.1e}), routing gap "
          f"{max(diag['route_gap']):.1e}; kernels:\n    " + "\n    ".join(tags) +
          "\n  error (rel-to-max): " + ", ".join(f"{k} {v:.2e}" for k, v in res.items()) + f"\n  worst {max(res.values()):.2e}")
    present, absent = exp[form]
    expect(tags, present, absent)
    for pattern, ncol, n in workers.get(form, []):
        hits = find(tags, pattern)
        assert hits, (pattern, tags)
        for t in hits:
            assert wave_strip_workers(t, ncol) == n, (t, n)
            if ncol <= 2:
                assert n % 8 != 0, t   # the plain strip map ran: the XCD-aware one needs workers % 8 == 0
    assert _lib.lib().pnpp_debug_wsd3_timeouts() == 0
    assert not wrong, wrong
    assert max(res.values()) <= GATE, res
