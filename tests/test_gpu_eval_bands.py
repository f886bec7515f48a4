"""GPU parity of the set-abstraction levels in EVAL mode (model.eval(): the validation pass that selects the checkpoint) across the
dispatcher's kernel bands, each case proving which kernels it ran -- tests/test_gpu_dispatch_bands.py and tests/test_gpu_cls_bands.py
with training=False at their band edges.  A short last validation batch (BankLoader keeps it) lands in another band than the full one.

Eval mode has code of its own (csrc/sa_api.hip: sa_forward_impl): BatchNorm is finalised from the running statistics BEFORE each product
(bn_finalize_fwd_kernel's eval branch) and the product goes out with E_STORE -- the E0 instantiation of every GEMM family; the pooled
GEMM epilogue is train-only (pool_here sits behind `if (!d->training) ... continue`), so pooling is always pool_fwd_kernel and
bn_finalize_fwd never carries +pool; gemm_mid3 needs E_STORE_STATS (try_launch_mid_gemm), so the split form runs gemm_mid as the mfma
form does; a level on raw coordinates finalises layer 0 with sa_fwd_finalize(L, 0, 0) and launches gemm_wsf03 / gemm_wsf0 without
moments (no rel_moments_kernel).  Backward, `training` only reaches the kernels' arithmetic (launch_bn_finalize_bwd, launch_post_gemm,
launch_xyz0_post: the BatchNorm transform degenerates to dZ = g istd dY, and d(conv bias) is no longer zero): no backward predicate
reads it, so the fused last-layer launch is the one the training case of the same shape takes -- gemm_wsd3 (split), gemm_wsp / gemm_wsq
(mfma; gemm_wsq's z-coefficient is exactly zero), gemm_ws<..,dW>, or the generic gemm_kernel / gemm_smallm / da_dw forms.

Each case: conftest.routed_level (classifier levels: the runner of test_gpu_cls_bands.py) with training=False, forward + backward,
every returned tensor within GATE = 1e-5 of its max-abs, route-gap and ReLU-margin assertions as they stand; the launch tags; worker
counts of the ragged / plain-map cases; running_mean / running_var bit-equal and num_batches_tracked unchanged across the pass;
pnpp_debug_wsd3_timeouts() == 0.  BatchNorm weight, bias and running statistics are moved off their defaults (uniform, as
test_sa1_shape_backward_in_eval_mode); the cases marked "var*" draw running_var log-uniformly over 1e-3 ... 1e2.  A case runs in both
float32 product forms only where its EVAL kernels differ: sa3 and the whole-cloud level differ in training by gemm_mid3 alone, so here
they run in the split form only.  Every case also asserts: no E1 (E_STORE_STATS) instantiation anywhere, no "+pool" on
bn_finalize_fwd, no gemm_mid3, no rel_moments_kernel.

The present / absent lists are derived from the predicates in csrc/ (named per row), written before the first GPU run.

  case (rows M)                predicate crossed                                      kernels asserted present (split | mfma) ; absent            worst error (split | mfma)
  sa1 S128 K32 D0 [64,64,128], N 1024, M = 4096 B
    sa1-B1      4096           sa_api.hip kSmallM; xyz0_applies / wsf_applies          gemm_kernel<64,64,2,2,A2,E0> (layer 0), gemm_smallm<A1,E0>   2.4e-7
                               M < 8192                                               N=64 / 128, pool_fwd, pool_bwd, +dZ, generic fused backward
                                                                                      gemm_smallm<A0,E2> K=128 ; wave-strip, gemm_ws, gemm_mid, da_dw
    sa1-B2 var* 8192           xyz0_applies / wsf_applies / wsd3_applies |            bn_finalize_fwd C=64 (sa_fwd_finalize(L,0,0)), gemm_wsf03<E0>  4.9e-7 | 3.6e-7
                               wsp_applies / wsx_applies: M >= 8192                   | gemm_wsf0<E0>, gemm_wsf3<64,A1,E0> | gemm_wsf<64,2,A1,E0>,
                                                                                      pool_fwd K=32, gemm_wsd3<128,32,A5> | gemm_wsp,
                                                                                      gemm_wsx<64,1,S3> | <64,1>, xyz0_post ; gemm_smallm,
                                                                                      gemm_kernel<, +dZ, gemm_ws, gemm_mid
    sa1-B5      20480          640 strips > 4 x 128 wsd3 workers: ragged rounds        as sa1-B2; gemm_wsd3<128> 128 workers                        2.9e-7 | 2.9e-7
    sa1-S43-B7  9632           301 strips, 76 workers (% 8 != 0: plain strip map);    as sa1-B2; 76 workers in every wave-strip kernel, pool_fwd    2.3e-7 | 3.3e-7
                               M % 64 = 32                                            G=301
  sa2 S32 K32 D128 [128,128,256], N 128, M = 1024 B, layer 0 convolved before the gather (sa_level_plan: delayed)
    sa2-B4      4096           kSmallM; mid_gemm_shape_ok: layer 2 only (256 tiles);  gather_rel_stats, gemm_smallm<A1,E0> N=128, gemm_mid<A1,E0>    3.0e-7
                               mid_da_dw_plan 136 tiles < 192                         N=256, pool_fwd, pool_bwd, da_dw_kernel<E2,A1> M=4096, +dZ,
                                                                                      scatter_dz ; wave-strip, gemm_kernel<, gemm_ws
    sa2-B5      5120           kSmallM < M < 8192; layer 1: 160 mid tiles < 192        gemm_kernel<64,64,2,2,A1,E0> N=128, gemm_mid<A1,E0> N=256,     2.8e-7
                                                                                      generic fused backward gemm_kernel<..,A5,E2>, <..,A4,E2> ;
                                                                                      wave-strip, gemm_smallm M=5120, da_dw M=5120, da_dw_mid, +dZ
    sa2-B7      7168           layer 1 reaches 224 mid tiles; try_launch_mid_da_dw    gemm_mid<A1,E0> N=128, N=256, gemm_kernel<..,A5,E2>,           3.7e-7
                               needs a materialised dZ (A_PLAIN)                      <..,A4,E2> ; as sa2-B5
    sa2-B8 var* 8192           wsf_applies, wsd3_applies | wsq_applies,               gemm_wsf3<128,A1,E0> N=128, N=256 | gemm_wsf<128,2,A1,E0>,     2.7e-7 | 5.6e-7
                               try_launch_ws Kd == 128: M >= 8192                     pool_fwd K=32 C=256, gemm_wsd3<256,32,A5> | gemm_wsq<256,
                                                                                      gemm_wsd3<128,32,A4> | gemm_ws<128,64,64,A4,E2,dW>,
                                                                                      gather_rel_stats, scatter_dz ; gemm_smallm M=8192,
                                                                                      gemm_kernel< M=8192, gemm_mid, +dZ
    sa2-B9      9216           288 strips: 36 wsf3 workers (plain map)                as sa2-B8, gemm_wsf3 grids 72 / 144                          2.5e-7 | 3.5e-7
    sa2-S43-B7  9632           301 strips: 38 wsf3 workers; M % 64 = 32: wsq_applies   gemm_wsf3 grids 76 / 152, gemm_wsd3 grids 256 | gemm_wsf,      2.2e-7 | 2.5e-7
                               false                                                  gemm_ws<256,64,64,A5,E2,dW> ; gemm_wsq
  sa3 group_all [256,512,1024], 32 rows per cloud, M = 32 B (split form only: try_launch_mid_gemm takes gemm_mid3 with E_STORE_STATS alone)
    sa3-B8      256            mid_gemm_shape_ok: M < 512; sa_bwd_top G <= 64          gemm_smallm<A3,E0> N=256, <A1,E0> N=512 / 1024, pool_fwd       2.5e-7
                                                                                      K=32, da_dw_kernel M=256, bn_finalize_bwd +dZ +pool ;
                                                                                      gemm_mid*, da_dw_mid, gemm_kernel<, pool_bwd, gemm_ws
    sa3-B24 var* 768           first mid_gemm_shape_ok shape of layer 2 (12 x 16);    gemm_mid<A1,E0> N=1024, gemm_smallm<A1,E0> N=512, pool_fwd,   5.1e-7
                               mid_da_dw_plan: layer 2 224 tiles, layer 1 80           da_dw_mid M=768, da_dw_kernel M=768, +dZ +pool ; gemm_mid3,
                                                                                      gemm_kernel<, pool_bwd
    sa3-B25     800            M % 64 != 0                                            gemm_smallm<A1,E0> N=1024, da_dw_kernel M=800, pool_fwd ;      2.8e-7
                                                                                      gemm_mid*, da_dw_mid, gemm_kernel<
    sa3-B128    4096           M == kSmallM; G = 128 > 64: pool_bwd launch             gemm_smallm<A3,E0> N=256, gemm_mid<A1,E0> N=512, N=1024,       7.4e-7
                                                                                      pool_fwd, da_dw_mid M=4096, pool_bwd, +dZ ; gemm_kernel<,
                                                                                      bwd +pool
    sa3-B129    4128           kSmallM < M, M % 64 != 0                               gemm_kernel<64,64,2,2,A3,E0>, <..,A1,E0> N=512, N=1024,        5.9e-7
                                                                                      <..,A5,E2>, pool_fwd, pool_bwd ; gemm_mid*, gemm_smallm,
                                                                                      da_dw, +dZ
    sa3-B256    8192           last mid_gemm_shape_ok shape; try_launch_ws Kd == 256   gemm_kernel<..,A3,E0>, gemm_ws<256,64,64,A1,E0>,               7.5e-7
                                                                                      gemm_mid<A1,E0> N=1024, gemm_kernel<..,A5,E2>, pool_fwd ;
                                                                                      gemm_smallm, da_dw
    sa3-B258    8256           past mid_gemm_shape_ok's upper bound                    gemm_ws<256,64,64,A1,E0>, gemm_kernel<..,A1,E0> N=1024,        7.3e-7
                                                                                      pool_fwd ; gemm_mid*, gemm_smallm, da_dw
  classifier level 1: D = 3, K = 32, [64,64,128], N = 256, radius 0.65
    l1-small    B2 S64  4096   kSmallM; launch_gemm M < 8192                           gemm_kernel<64,64,2,2,A2,E0> K=8, gemm_smallm<A1,E0> N=64 /    2.7e-7
                                                                                      128, gemm_smallm N=3 (dF), +dZ, pool_fwd, pool_bwd ;
                                                                                      wave-strip, gemm_ws, da_dw
    l1-ragged   B7 S43  9632   wsf_applies, wsd3_applies | wsp_applies; 76 workers     gemm_kernel<..,A2,E0>, gemm_wsf3<64,A1,E0> N=64, N=128 |       2.6e-7 | 2.6e-7
                               (plain map); try_launch_ws Kd == 64 (dA + dW)          gemm_wsf<64,2,A1,E0>, gemm_wsd3<128,32,A5> | gemm_wsp,
                                                                                      gemm_ws<64,64,64,A4,E2,dW>, pool_fwd K=32 ; gemm_wsx,
                                                                                      xyz0_post, gemm_wsf03, gemm_wsf0, gemm_smallm
  classifier level 2: D = 128, K = 64, [128,128,256], N = 128, radius 1.1
    l2-small var* B2 S32 4096  kSmallM; mid_gemm_shape_ok layer 2; sa_bwd_top G = 64   gather_rel_stats, gemm_smallm<A1,E0> N=128, gemm_mid<A1,E0>    3.8e-7
                                                                                      N=256, pool_fwd K=64, da_dw_kernel M=4096, +dZ +pool,
                                                                                      scatter_dz ; wave-strip, gemm_kernel<, gemm_ws, pool_bwd
    l2-mid      B2 S40  5120   kSmallM < M < 8192; layer 1 160 mid tiles               gemm_kernel<64,64,2,2,A1,E0> N=128, gemm_mid<A1,E0> N=256,     3.4e-7
                                                                                      gemm_kernel<..,A5,E2>, <..,A4,E2>, pool_fwd, pool_bwd ;
                                                                                      wave-strip, gemm_ws, gemm_smallm M=5120, da_dw M=5120, +dZ
    l2-ragged   B3 S43  8256   wsf_applies; wsd3_applies dense | try_launch_ws; every  gemm_wsf3<128,A1,E0> N=128, N=256 | gemm_wsf<128,2,A1,E0>,     2.2e-7 | 2.7e-7
                               K == 32 predicate false (wsq, wsp, wsd3 pooled)        gemm_wsd3<128,32,A4> | gemm_ws<128,64,64,A4,E2,dW>,
                                                                                      gemm_ws<256,64,64,A5,E2,dW>, pool_fwd K=64, pool_bwd K=64 ;
                                                                                      gemm_wsq, gemm_wsp, gemm_wsd3<256, gemm_wsd3<128,32,A5>
    l2-gathered B64 S2  8192   sa_level_plan: S K = N, not delayed; try_launch_ws      gemm_ws<132,64,64,A2,E0> (layer 0), layers 1-2 as l2-ragged,   2.8e-7 | 2.8e-7
                               gather form D == 128                                   gemm_ws<128,64,64,A4,E0> + scatter_rows_bwd C=128 (dF) ;
                                                                                      gather_rel_stats, scatter_dz, da_dw
  whole cloud: 128 rows per cloud, [256,512,1024]; pool_fwd_kernel K=128 in every case (split form only, as sa3)
    ga-B3       384            mid_gemm_shape_ok / mid_da_dw_plan: M < 512             gemm_smallm<..,E0> N=256 / 512 / 1024, da_dw_kernel M=384,     2.7e-7
                                                                                      +dZ +pool ; gemm_mid*, da_dw_mid, gemm_kernel<, gemm_ws
    ga-B6       768            first mid shape of layer 2                              gemm_mid<A1,E0> N=1024, gemm_smallm N=256 / 512, da_dw_mid     3.5e-7
                                                                                      M=768, da_dw_kernel M=768, +dZ +pool ; gemm_mid3
    ga-B32      4096           M == kSmallM; G = 32 <= 64                              gemm_smallm N=256, gemm_mid<A1,E0> N=512, N=1024, da_dw_mid,   6.6e-7
                                                                                      da_dw_kernel<E0,A3>, +dZ +pool ; gemm_kernel<, pool_bwd
    ga-B33      4224           past kSmallM, M % 64 == 0                               gemm_kernel<..,A3,E0>, gemm_mid<A1,E0> N=512, N=1024,          6.1e-7
                                                                                      gemm_kernel<..,A5,E2>, <..,A4,E2>, pool_bwd K=128 ;
                                                                                      gemm_smallm, da_dw, +dZ
    ga-B64      8192           last mid_gemm_shape_ok shape; try_launch_ws Kd == 256   gemm_kernel<..,A3,E0>, gemm_ws<256,64,64,A1,E0>, gemm_mid      5.2e-7
                                                                                      N=1024, gemm_kernel<..,A5,E2>, gemm_ws<256,64,64,A4,E0> (dF)
    ga-B65      8320           past mid_gemm_shape_ok                                  gemm_ws<256,64,64,A1,E0>, gemm_kernel<..,A1,E0> N=1024 ;       5.9e-7
                                                                                      gemm_mid*, gemm_smallm, da_dw

Property tests (forward only, on sa1-B2, sa2-B8, sa3-B24, l2-small): the validation path -- the same forward under torch.no_grad()
launches the same tags and returns bit-equal output -- and batch independence: cloud 0 run alone (B = 1: another band for sa1 and sa2)
finds the same neighbours and agrees with row 0 of the batched output within 2 GATE max|y64| (both sides lie within GATE of the same
float64 value; eval-mode BatchNorm does not couple the clouds).

Measured on the MI355X (rel-to-max, worst tensor of the case): sa1 2.3e-7 ... 4.9e-7, sa2 2.2e-7 ... 5.6e-7, sa3 2.5e-7 ... 7.5e-7,
classifier level 1 2.6e-7 ... 2.7e-7, level 2 2.2e-7 ... 3.8e-7, whole cloud 2.7e-7 ... 6.6e-7; the var* cases held the full 1e-3 ... 1e2
range (no ReLU decision further than 6.1e-8 from float64's own, routing gap <= 6.7e-16).  Batch independence: cloud 0 alone against row 0
of the batch 2.4e-7 ... 4.6e-7 of max|y64| (bound 2e-5).  The first run agreed with every present / absent list.  Mutation (not
committed): the eval-only d(conv bias) scale of bn_finalize_bwd_block times 1.0002 fails all 38 band cases at 2.0e-4 while
tests/test_gpu_dispatch_bands.py passes unchanged.
"""
import re

import pytest
import torch

from conftest import relmax, routed_level, tap_to_routing
from dispatch import expect, find, record, wave_strip_workers
from test_gpu_cls_bands import FAMILY, _inputs as cls_inputs, _members, _routed as cls_routed
from test_gpu_dispatch_bands import _inputs as sa_inputs
from test_gpu_levels_routed import GATE

pytestmark = pytest.mark.gpu

SA1, SA2, SA3 = (128, 32, 0, [64, 64, 128], 1024), (32, 32, 128, [128, 128, 256], 128), (None, None, 256, [256, 512, 1024], 32)
SA1_S43, SA2_S43 = (43, 32, 0, [64, 64, 128], 1024), (43, 32, 128, [128, 128, 256], 128)
BOTH, SPLIT = ("split", "mfma"), ("split",)
VAR_DECADES = (-3.0, 2.0)   # log10 range of running_var in the "var*" cases

WAVE_STRIP = ["gemm_wsf03", "gemm_wsf0_", "gemm_wsf3", "gemm_wsf_", "gemm_wsd3", "gemm_wsp", "gemm_wsq", "gemm_wsx", "xyz0_post"]
MID = ["gemm_mid_kernel", "da_dw_mid_kernel"]
FWD_POOL, BWD_POOL, DZ = "bn_finalize_fwd_kernel +pool", "bn_finalize_bwd_kernel +pool", "bn_finalize_bwd_kernel +dZ"
# what no eval-mode pass launches (sa_forward_impl's `if (!d->training)` branches; try_launch_mid_gemm: gemm_mid3 needs E_STORE_STATS)
EVAL_NEVER = [FWD_POOL, "gemm_mid3_kernel", "rel_moments_kernel"]
# a level with features never takes the coordinate-level shortcut (xyz0_applies / wsx_applies: D == 0)
NO_XYZ0 = ["gemm_wsx", "xyz0_post", "gemm_wsf03", "gemm_wsf0_"]
# level 2 of the classifier (K = 64): wsq_applies, wsp_applies and the pooled branch of wsd3_applies test A.K == 32
L2_NEVER = ["gemm_wsq", "gemm_wsp", "gemm_wsd3_kernel<256", "gemm_wsd3_kernel<128,32,A5>"] + NO_XYZ0


def _forms(split, mfma, present=(), absent=()):
    """{form: (present, absent)}: the form's own kernels, the other form's kernel families among the absent ones"""
    return {"split": (list(split) + list(present), [t.split()[0] for t in mfma if t not in split] + list(absent)),
            "mfma": (list(mfma) + list(present), [t.split()[0] for t in split if t not in mfma] + list(absent))}


def _same(present, absent=()):
    return {"split": (list(present), list(absent)), "mfma": (list(present), list(absent))}


def _sa1_ws(M):
    """sa1 at M >= 8192 (xyz0_applies): layer 0 from the coordinates, finalised from the running statistics by a launch of its own"""
    split = [f"gemm_wsf03_kernel<E0> M={M}", f"gemm_wsf3_kernel<64,A1,E0> M={M} N=128", "gemm_wsd3_kernel<128,32,A5>", "gemm_wsx_kernel<64,1,S3>"]
    mfma = [f"gemm_wsf0_kernel<E0> M={M}", f"gemm_wsf_kernel<64,2,A1,E0> M={M} N=128", "gemm_wsp_kernel", "gemm_wsx_kernel<64,1>"]
    return _forms(split, mfma, ["bn_finalize_fwd_kernel C=64", "bn_finalize_fwd_kernel C=128", "pool_fwd_kernel K=32 C=128", "pool_bwd_kernel K=32",
                                "xyz0_post_kernel"],
                  ["gemm_smallm", "gemm_kernel<", DZ, BWD_POOL, "gemm_ws_kernel", "gemm_mid", "da_dw", "gemm_wsq"])


def _sa2_ws(M, wsq=True):
    """sa2 at M >= 8192; wsq_applies needs M % 64 == 0, else the mfma form's last-layer backward is gemm_ws<256,..,dW>"""
    split = [f"gemm_wsf3_kernel<128,A1,E0> M={M} N=128", f"gemm_wsf3_kernel<128,A1,E0> M={M} N=256", "gemm_wsd3_kernel<256,32,A5>",
             "gemm_wsd3_kernel<128,32,A4>"]
    mfma = [f"gemm_wsf_kernel<128,2,A1,E0> M={M} N=128", f"gemm_wsf_kernel<128,2,A1,E0> M={M} N=256",
            "gemm_wsq_kernel<256" if wsq else "gemm_ws_kernel<256,64,64,A5,E2,dW>", "gemm_ws_kernel<128,64,64,A4,E2,dW>"]
    return _forms(split, mfma, ["gather_rel_stats_kernel", "scatter_dz_kernel", "pool_fwd_kernel K=32 C=256", "pool_bwd_kernel K=32"],
                  [f"gemm_smallm_kernel M={M}", f"gemm_kernel< M={M}", "gemm_mid", DZ, BWD_POOL, "gemm_wsp"] + NO_XYZ0 + ([] if wsq else ["gemm_wsq"]))


def _l1_ws(M):
    """classifier level 1 at M >= 8192: layer 0 on the chunked kernel (D = 3), dF through the generic GEMM and the row scatter"""
    split = [f"gemm_wsf3_kernel<64,A1,E0> M={M} N=64", f"gemm_wsf3_kernel<64,A1,E0> M={M} N=128", "gemm_wsd3_kernel<128,32,A5>"]
    mfma = [f"gemm_wsf_kernel<64,2,A1,E0> M={M} N=64", f"gemm_wsf_kernel<64,2,A1,E0> M={M} N=128", "gemm_wsp_kernel"]
    return _forms(split, mfma, [f"gemm_kernel<64,64,2,2,A2,E0> M={M} N=64 K=8", "gemm_ws_kernel<64,64,64,A4,E2,dW>", "dw_kernel<A4,A2>",
                                "pool_fwd_kernel K=32", "pool_bwd_kernel K=32", "gemm_kernel<128,32,4,1,A4,E0> N=3", "scatter_rows_bwd_kernel C=3"],
                  NO_XYZ0 + ["gather_rel_stats", "scatter_dz", "gemm_wsq", "gemm_mid", "da_dw", "gemm_smallm", BWD_POOL, DZ])


def _l2_ws(M, gathered=False):
    """classifier level 2 at M >= 8192"""
    split = [f"gemm_wsf3_kernel<128,A1,E0> M={M} N=128", f"gemm_wsf3_kernel<128,A1,E0> M={M} N=256", "gemm_wsd3_kernel<128,32,A4>"]
    mfma = [f"gemm_wsf_kernel<128,2,A1,E0> M={M} N=128", f"gemm_wsf_kernel<128,2,A1,E0> M={M} N=256", "gemm_ws_kernel<128,64,64,A4,E2,dW>"]
    present = ["gemm_ws_kernel<256,64,64,A5,E2,dW>", "pool_fwd_kernel K=64", "pool_bwd_kernel K=64"]
    absent = L2_NEVER + [f"gemm_smallm_kernel M={M}", "gemm_kernel<", "gemm_mid", BWD_POOL, DZ]
    if gathered:
        present += ["gemm_ws_kernel<132,64,64,A2,E0>", "dw_kernel<A4,A2>", "gemm_ws_kernel<128,64,64,A4,E0>", "scatter_rows_bwd_kernel C=128"]
        absent += ["gather_rel_stats", "scatter_dz", "da_dw"]
    else:
        present += ["gather_rel_stats_kernel", "scatter_dz_kernel", "da_dw_kernel<E0,A0>"]
    return _forms(split, mfma, present, absent)


def _sa3(rows, present, absent):
    """a whole-cloud level (sa3: 32 rows per cloud, the classifier's: 128): pooling is always a pool_fwd_kernel over the cloud"""
    return _same([f"pool_fwd_kernel K={rows}"] + list(present), ["pool_fwd_split"] + WAVE_STRIP + list(absent))


def _w(n, split, mfma=()):
    """worker-count checks {form: [(pattern, column blocks, workers, plain strip map)]}; plain: workers % 8 != 0 (no XCD-aware map)"""
    return {"split": [(p, c, n if w is None else w, (n if w is None else w) % 8 != 0) for p, c, w in split],
            "mfma": [(p, c, n if w is None else w, (n if w is None else w) % 8 != 0) for p, c, w in mfma]}


# case id -> (kind, geometry, B, product forms, {form: (present, absent)}, worker checks, running_var over VAR_DECADES)
#   kind "sa1" / "sa2" / "sa3": PointNetSetAbstraction through conftest.routed_level, geometry (S, K, D, mlp, N)
#   kind "cls": a classifier level through test_gpu_cls_bands' runner; family, B and S are that file's case of the same id
CASES = {
    "sa1-B1": ("sa1", SA1, 1, SPLIT,
               _same(["gemm_kernel<64,64,2,2,A2,E0> M=4096 N=64 K=4", "gemm_smallm_kernel<A1,E0,T1> M=4096 N=64", "gemm_smallm_kernel<A1,E0,T1> M=4096 N=128",
                      "gemm_smallm_kernel<A0,E2,T0> M=4096 N=64 K=128", "pool_fwd_kernel K=32 C=128", "pool_bwd_kernel K=32", DZ],
                     WAVE_STRIP + ["gemm_ws_kernel", "gemm_mid", "da_dw", BWD_POOL]), {}, False),
    "sa1-B2": ("sa1", SA1, 2, BOTH, _sa1_ws(8192), {}, True),
    "sa1-B5": ("sa1", SA1, 5, BOTH, _sa1_ws(20480), _w(128, [("gemm_wsd3_kernel<128", 2, None)]), False),
    "sa1-S43-B7": ("sa1", SA1_S43, 7, BOTH, {f: (p + ["pool_fwd_kernel G=301"], a) for f, (p, a) in _sa1_ws(9632).items()},
                   _w(76, [("gemm_wsf03_kernel", 1, None), ("gemm_wsf3_kernel<64", 2, None), ("gemm_wsd3_kernel<128", 2, None), ("gemm_wsx_kernel", 1, None)],
                      [("gemm_wsf0_kernel", 1, None), ("gemm_wsf_kernel<64", 2, None), ("gemm_wsp_kernel", 1, None), ("gemm_wsx_kernel", 1, None)]), False),
    "sa2-B4": ("sa2", SA2, 4, SPLIT,
               _same(["gather_rel_stats_kernel", "gemm_smallm_kernel<A1,E0,T1> M=4096 N=128", "gemm_mid_kernel<A1,E0,T1> M=4096 N=256",
                      "pool_fwd_kernel K=32 C=256", "pool_bwd_kernel K=32", "da_dw_kernel<E2,A1> M=4096", DZ, "scatter_dz_kernel"],
                     WAVE_STRIP + ["gemm_kernel<", "gemm_ws_kernel", "da_dw_mid", BWD_POOL]), {}, False),
    "sa2-B5": ("sa2", SA2, 5, SPLIT,
               _same(["gather_rel_stats_kernel", "gemm_kernel<64,64,2,2,A1,E0> M=5120 N=128", "gemm_mid_kernel<A1,E0,T1> M=5120 N=256",
                      "pool_fwd_kernel K=32 C=256", "pool_bwd_kernel K=32", "gemm_kernel<64,64,2,2,A5,E2> M=5120", "gemm_kernel<64,64,2,2,A4,E2> M=5120",
                      "scatter_dz_kernel"],
                     WAVE_STRIP + ["gemm_smallm_kernel M=5120", "da_dw_kernel M=5120", "da_dw_mid", "gemm_ws_kernel", DZ, BWD_POOL]), {}, False),
    "sa2-B7": ("sa2", SA2, 7, SPLIT,
               _same(["gather_rel_stats_kernel", "gemm_mid_kernel<A1,E0,T1> M=7168 N=128", "gemm_mid_kernel<A1,E0,T1> M=7168 N=256",
                      "pool_fwd_kernel K=32 C=256", "pool_bwd_kernel K=32", "gemm_kernel<64,64,2,2,A5,E2> M=7168", "gemm_kernel<64,64,2,2,A4,E2> M=7168",
                      "scatter_dz_kernel"],
                     WAVE_STRIP + ["gemm_smallm_kernel M=7168", "da_dw_kernel M=7168", "da_dw_mid", "gemm_ws_kernel", DZ, BWD_POOL]), {}, False),
    "sa2-B8": ("sa2", SA2, 8, BOTH, _sa2_ws(8192), {}, True),
    "sa2-B9": ("sa2", SA2, 9, BOTH, _sa2_ws(9216),
               _w(36, [("gemm_wsf3_kernel<128 M=9216 N=128", 2, None), ("gemm_wsf3_kernel<128 M=9216 N=256", 4, None)]), False),
    "sa2-S43-B7": ("sa2", SA2_S43, 7, BOTH, _sa2_ws(9632, wsq=False),
                   _w(38, [("gemm_wsf3_kernel<128 M=9632 N=128", 2, None), ("gemm_wsf3_kernel<128 M=9632 N=256", 4, None),
                           ("gemm_wsd3_kernel<256", 4, 64), ("gemm_wsd3_kernel<128", 4, 64)]), False),
    "sa3-B8": ("sa3", SA3, 8, SPLIT,
               _sa3(32, ["gemm_smallm_kernel<A3,E0,T1> M=256 N=256", "gemm_smallm_kernel<A1,E0,T1> M=256 N=512", "gemm_smallm_kernel<A1,E0,T1> M=256 N=1024",
                         "da_dw_kernel<E2,A1> M=256", "da_dw_kernel<E0,A3> M=256", DZ + " +pool"],
                    MID + ["gemm_kernel<", "pool_bwd_kernel", "gemm_ws_kernel"]), {}, False),
    "sa3-B24": ("sa3", SA3, 24, SPLIT,
                _sa3(32, ["gemm_smallm_kernel<A3,E0,T1> M=768 N=256", "gemm_smallm_kernel<A1,E0,T1> M=768 N=512", "gemm_mid_kernel<A1,E0,T1> M=768 N=1024",
                          "da_dw_mid_kernel<E2,A1> M=768", "da_dw_kernel<E2,A1> M=768", DZ + " +pool"],
                     ["gemm_kernel<", "pool_bwd_kernel", "gemm_ws_kernel", "gemm_smallm_kernel M=768 N=1024"]), {}, True),
    "sa3-B25": ("sa3", SA3, 25, SPLIT,
                _sa3(32, ["gemm_smallm_kernel<A1,E0,T1> M=800 N=512", "gemm_smallm_kernel<A1,E0,T1> M=800 N=1024", "da_dw_kernel<E2,A1> M=800", DZ + " +pool"],
                     MID + ["gemm_kernel<", "pool_bwd_kernel", "gemm_ws_kernel"]), {}, False),
    "sa3-B128": ("sa3", SA3, 128, SPLIT,
                 _sa3(32, ["gemm_smallm_kernel<A3,E0,T1> M=4096 N=256", "gemm_mid_kernel<A1,E0,T1> M=4096 N=512", "gemm_mid_kernel<A1,E0,T1> M=4096 N=1024",
                           "da_dw_mid_kernel<E2,A1> M=4096", "da_dw_kernel<E0,A3> M=4096", "pool_bwd_kernel K=32", DZ],
                      ["gemm_kernel<", "gemm_ws_kernel", BWD_POOL]), {}, False),
    "sa3-B129": ("sa3", SA3, 129, SPLIT,
                 _sa3(32, ["gemm_kernel<64,64,2,2,A3,E0> M=4128", "gemm_kernel<64,64,2,2,A1,E0> M=4128 N=512", "gemm_kernel<64,64,2,2,A1,E0> M=4128 N=1024",
                           "gemm_kernel<64,64,2,2,A5,E2> M=4128", "gemm_kernel<64,64,2,2,A4,E2> M=4128", "pool_bwd_kernel K=32"],
                      MID + ["gemm_smallm", "da_dw", "gemm_ws_kernel", DZ, BWD_POOL]), {}, False),
    "sa3-B256": ("sa3", SA3, 256, SPLIT,
                 _sa3(32, ["gemm_kernel<64,64,2,2,A3,E0> M=8192", "gemm_ws_kernel<256,64,64,A1,E0> M=8192", "gemm_mid_kernel<A1,E0,T1> M=8192 N=1024",
                           "gemm_kernel<64,64,2,2,A5,E2> M=8192", "gemm_kernel<64,64,2,2,A4,E2> M=8192", "pool_bwd_kernel K=32"],
                      ["gemm_smallm", "da_dw", DZ, BWD_POOL, "gemm_mid_kernel M=8192 N=512"]), {}, False),
    "sa3-B258": ("sa3", SA3, 258, SPLIT,
                 _sa3(32, ["gemm_kernel<64,64,2,2,A3,E0> M=8256", "gemm_ws_kernel<256,64,64,A1,E0> M=8256", "gemm_kernel<64,64,2,2,A1,E0> M=8256 N=1024",
                           "gemm_kernel<64,64,2,2,A5,E2> M=8256", "pool_bwd_kernel K=32"],
                      MID + ["gemm_smallm", "da_dw", DZ, BWD_POOL]), {}, False),
    "l1-small": ("cls", None, None, SPLIT,
                 _same(["gemm_kernel<64,64,2,2,A2,E0> M=4096 N=64 K=8", "gemm_smallm_kernel<A1,E0,T1> M=4096 N=64", "gemm_smallm_kernel<A1,E0,T1> M=4096 N=128",
                        "gemm_smallm_kernel<A0,E2,T0> M=4096 N=64 K=128", "gemm_smallm_kernel M=4096 N=3", "scatter_rows_bwd_kernel C=3", DZ,
                        "pool_fwd_kernel K=32", "pool_bwd_kernel K=32"],
                       WAVE_STRIP + ["gather_rel_stats", "scatter_dz", "gemm_mid", "da_dw", "gemm_ws_kernel", BWD_POOL]), {}, False),
    "l1-ragged": ("cls", None, None, BOTH, _l1_ws(9632),
                  _w(76, [("gemm_wsf3_kernel<64 M=9632 N=64", 1, None), ("gemm_wsf3_kernel<64 M=9632 N=128", 2, None), ("gemm_wsd3_kernel<128", 2, None)],
                     [("gemm_wsf_kernel<64 M=9632 N=64", 1, None), ("gemm_wsf_kernel<64 M=9632 N=128", 2, None), ("gemm_wsp_kernel", 1, None)]), False),
    "l2-small": ("cls", None, None, SPLIT,
                 _same(["gather_rel_stats_kernel", "gemm_smallm_kernel<A1,E0,T1> M=4096 N=128", "gemm_mid_kernel<A1,E0,T1> M=4096 N=256", "pool_fwd_kernel K=64",
                        "da_dw_kernel<E2,A1> M=4096", DZ + " +pool", "scatter_dz_kernel"],
                       WAVE_STRIP + ["gemm_kernel<", "gemm_ws_kernel", "pool_bwd_kernel", "da_dw_mid"]), {}, True),
    "l2-mid": ("cls", None, None, SPLIT,
               _same(["gather_rel_stats_kernel", "gemm_kernel<64,64,2,2,A1,E0> M=5120 N=128", "gemm_mid_kernel<A1,E0,T1> M=5120 N=256", "pool_fwd_kernel K=64",
                      "pool_bwd_kernel K=64", "gemm_kernel<64,64,2,2,A5,E2> M=5120", "gemm_kernel<64,64,2,2,A4,E2> M=5120", "dw_kernel<A5,A1>",
                      "dw_kernel<A4,A1>", "scatter_dz_kernel"],
                     WAVE_STRIP + ["gemm_ws_kernel", "gemm_smallm_kernel M=5120", "da_dw_kernel M=5120", "da_dw_mid", BWD_POOL, DZ]), {}, False),
    "l2-ragged": ("cls", None, None, BOTH, _l2_ws(8256),
                  _w(33, [("gemm_wsf3_kernel<128 M=8256 N=128", 2, None), ("gemm_wsf3_kernel<128 M=8256 N=256", 4, None), ("gemm_wsd3_kernel<128", 4, 64)]), False),
    "l2-gathered": ("cls", None, None, BOTH, _l2_ws(8192, gathered=True), {}, False),
    "ga-B3": ("cls", None, None, SPLIT,
              _sa3(128, ["gemm_smallm_kernel<A3,E0,T1> M=384 N=256", "gemm_smallm_kernel<A1,E0,T1> M=384 N=512", "gemm_smallm_kernel<A1,E0,T1> M=384 N=1024",
                         "da_dw_kernel<E2,A1> M=384", DZ + " +pool"], MID + ["gemm_kernel<", "gemm_ws_kernel", "pool_bwd_kernel"]), {}, False),
    "ga-B6": ("cls", None, None, SPLIT,
              _sa3(128, ["gemm_smallm_kernel<A3,E0,T1> M=768 N=256", "gemm_smallm_kernel<A1,E0,T1> M=768 N=512", "gemm_mid_kernel<A1,E0,T1> M=768 N=1024",
                         "da_dw_mid_kernel<E2,A1> M=768", "da_dw_kernel<E2,A1> M=768", DZ + " +pool"],
                   ["gemm_kernel<", "gemm_ws_kernel", "pool_bwd_kernel"]), {}, False),
    "ga-B32": ("cls", None, None, SPLIT,
               _sa3(128, ["gemm_smallm_kernel<A3,E0,T1> M=4096 N=256", "gemm_mid_kernel<A1,E0,T1> M=4096 N=512", "gemm_mid_kernel<A1,E0,T1> M=4096 N=1024",
                          "da_dw_mid_kernel<E2,A1> M=4096", "da_dw_kernel<E0,A3> M=4096", DZ + " +pool"],
                    ["gemm_kernel<", "gemm_ws_kernel", "pool_bwd_kernel"]), {}, False),
    "ga-B33": ("cls", None, None, SPLIT,
               _sa3(128, ["gemm_kernel<64,64,2,2,A3,E0> M=4224", "gemm_mid_kernel<A1,E0,T1> M=4224 N=512", "gemm_mid_kernel<A1,E0,T1> M=4224 N=1024",
                          "gemm_kernel<64,64,2,2,A5,E2> M=4224", "gemm_kernel<64,64,2,2,A4,E2> M=4224", "gemm_kernel<64,64,2,2,A4,E0> M=4224",
                          "pool_bwd_kernel K=128"], ["gemm_smallm", "da_dw", DZ, BWD_POOL, "gemm_ws_kernel"]), {}, False),
    "ga-B64": ("cls", None, None, SPLIT,
               _sa3(128, ["gemm_kernel<64,64,2,2,A3,E0> M=8192", "gemm_ws_kernel<256,64,64,A1,E0> M=8192", "gemm_mid_kernel<A1,E0,T1> M=8192 N=1024",
                          "gemm_kernel<64,64,2,2,A5,E2> M=8192", "gemm_kernel<64,64,2,2,A4,E2> M=8192", "gemm_ws_kernel<256,64,64,A4,E0> M=8192",
                          "pool_bwd_kernel K=128"], ["gemm_smallm", "da_dw", DZ, BWD_POOL, "gemm_mid_kernel M=8192 N=512"]), {}, False),
    "ga-B65": ("cls", None, None, SPLIT,
               _sa3(128, ["gemm_kernel<64,64,2,2,A3,E0> M=8320", "gemm_ws_kernel<256,64,64,A1,E0> M=8320", "gemm_kernel<64,64,2,2,A1,E0> M=8320 N=1024",
                          "gemm_kernel<64,64,2,2,A5,E2> M=8320", "gemm_ws_kernel<256,64,64,A4,E0> M=8320", "pool_bwd_kernel K=128"],
                    MID + ["gemm_smallm", "da_dw", BWD_POOL]), {}, False),
}
PROPERTY_CASES = ["sa1-B2", "sa2-B8", "sa3-B24", "l2-small"]


@pytest.fixture()
def products():
    from pnpp_hip import ops
    before = ops.get_float32_products()
    yield ops
    ops.set_float32_products(before)


def _bns(module):
    return list(module.bns if hasattr(module, "bns") else module.mlp_bns)


def _module(cid):
    """the case's level in eval mode, BatchNorm affine parameters and running statistics off their defaults"""
    kind, geo, _, _, _, _, wide = CASES[cid]
    torch.manual_seed(5000 + list(CASES).index(cid))
    if kind == "cls":
        from models.pointnet_pp_cls import SimpleSetAbstraction, SimpleSetAbstractionGroupAll
        from test_gpu_cls_bands import CASES as CLS
        fam, _, S = CLS[cid][:3]
        K, D, mlp, _, radius, _ = FAMILY[fam]
        module = SimpleSetAbstractionGroupAll(D, list(mlp)) if fam == "ga" else SimpleSetAbstraction(S, radius, K, D, list(mlp))
    else:
        from models.pointnet_pp_8dir import PointNetSetAbstraction
        S, K, D, mlp, _ = geo
        module = PointNetSetAbstraction(S, K, D, list(mlp), group_all=S is None)
    with torch.no_grad():
        for bn in _bns(module):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
            bn.running_mean.uniform_(-0.2, 0.2)
            if wide:
                bn.running_var.copy_(10.0 ** torch.empty_like(bn.running_var).uniform_(*VAR_DECADES))
            else:
                bn.running_var.uniform_(0.5, 1.5)
    return module.cuda().eval()


def _setup(cid, ops):
    """-> module, (xyz, pts, centres, gy), neighbour lists of the radius query (classifier levels) or None, K, group_all, rows M"""
    kind, geo, B, _, _, _, _ = CASES[cid]
    module = _module(cid)
    if kind != "cls":
        S, K, _, _, N = geo
        seed = 2000 + B + 7 * (S or 0)
        return module, sa_inputs(kind, geo, B, seed), None, K, S is None, B * (S or 1) * (K or N)
    from test_gpu_cls_bands import CASES as CLS
    fam, B, S = CLS[cid][:3]
    K, _, _, N, _, _ = FAMILY[fam]
    xyz, pts, centres, gy, radius = cls_inputs(cid)
    if fam == "ga":
        return module, (xyz, pts, None, gy), None, K, True, B * N
    xg = xyz.cuda()
    nbr = ops.ball_query(radius, K, xg, ops.index_points(xg, centres.cuda()))
    n = _members(nbr.cpu())
    assert bool((n == K).any()) and bool((n < K).any()), "the radius must leave full and padded neighbourhoods"
    return module, (xyz, pts, centres, gy), nbr, K, False, B * S * K


def _forward(cid, module, xyz, pts, centres, nbr, K, group_all):
    """the level's forward pass on the HIP kernels -> output (B, S or 1, C)"""
    if CASES[cid][0] != "cls":
        return module(xyz.cuda(), None if pts is None else pts.cuda(), None if group_all else centres.cuda())[1]
    from pnpp_hip import ops
    return ops.set_abstraction(xyz.cuda(), pts.cuda(), None if group_all else centres.to(torch.int32).cuda(), None if group_all else K, group_all,
                               False, module.mlp_convs, module.mlp_bns, neighbour_idx=nbr)[1]


def _tapped(fn):
    """fn() with ops.sa_tap armed -> (fn's result, the call's routing)"""
    from pnpp_hip import ops
    ops.sa_tap = []
    try:
        y = fn()
        return y, tap_to_routing(ops.sa_tap)[0]
    finally:
        ops.sa_tap = None


PARAMS = [pytest.param(cid, form, id=f"{cid}-{form}") for cid, c in CASES.items() for form in c[3]]


@pytest.mark.parametrize("cid,form", PARAMS)
def test_band(oracle, products, cid, form):
    from pnpp_hip import _lib
    kind, _, _, _, exp, workers, _ = CASES[cid]
    products.set_float32_products(form)
    module, (xyz, pts, centres, gy), nbr, K, group_all, M = _setup(cid, products)
    assert not module.training
    before = [(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)) for bn in _bns(module)]
    out = {}
    if kind == "cls":
        tags = record(lambda: out.update(r=cls_routed(oracle, module, xyz, pts, centres, nbr, gy, K, group_all, False)))
        res, diag, wrong = out["r"]
    else:
        tags = record(lambda: out.update(r=routed_level(oracle, module, xyz, pts, centres, gy, K, group_all, training=False)))
        (res, diag), wrong = out["r"], []
    torch.cuda.synchronize()
    print(f"\n[{cid} {form}] M={M} ReLU flips {diag['relu_flips']} (margin {max(diag['relu_flip_margin']):.1e}), routing gap "
          f"{max(diag['route_gap']):.1e}; kernels:\n    " + "\n    ".join(tags) +
          "\n  error (rel-to-max): " + ", ".join(f"{k} {v:.2e}" for k, v in res.items()) + f"\n  worst {max(res.values()):.2e}")
    present, absent = exp[form]
    expect(tags, present, absent + EVAL_NEVER)
    stats = [t for t in tags if re.search(r"[<,]E1[,>]", t.split()[0])]
    assert not stats, ("an eval-mode pass launched a statistics epilogue (E_STORE_STATS)", stats)
    for pattern, ncol, n, plain in workers.get(form, []):
        hits = find(tags, pattern)
        assert hits, (pattern, tags)
        for t in hits:
            assert wave_strip_workers(t, ncol) == n, (t, n)
            if plain:
                assert n % 8 != 0, t   # the plain strip map ran: the XCD-aware one needs workers % 8 == 0
    for l, (bn, (rm, rv, nbt)) in enumerate(zip(_bns(module), before)):
        assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv), f"bns.{l}: an eval-mode pass wrote to the running statistics"
        assert int(bn.num_batches_tracked) == nbt, f"bns.{l}.num_batches_tracked {int(bn.num_batches_tracked)} != {nbt}"
    assert _lib.lib().pnpp_debug_wsd3_timeouts() == 0
    assert not wrong, wrong
    # with running statistics the layer is affine: the conv bias has a gradient of its own (exactly zero, and skipped, in training)
    assert set(res) >= {"out"} | ({"d_points"} if pts is not None else set()) | {f"d_convs.{l}.bias" for l in range(len(before))}, sorted(res)
    assert max(res.values()) <= GATE, res


@pytest.mark.parametrize("cid", PROPERTY_CASES)
def test_validation_path_under_no_grad(products, cid):
    """The validation loop runs under torch.no_grad(): the same launches, bit-equal output."""
    products.set_float32_products("split")
    module, (xyz, pts, centres, _), nbr, K, group_all, _ = _setup(cid, products)
    out = {}
    tags = record(lambda: out.update(y=_forward(cid, module, xyz, pts, centres, nbr, K, group_all)))
    with torch.no_grad():
        tags_ng = record(lambda: out.update(y_ng=_forward(cid, module, xyz, pts, centres, nbr, K, group_all)))
    assert out["y"].requires_grad and not out["y_ng"].requires_grad
    assert tags == tags_ng, (tags, tags_ng)
    assert torch.equal(out["y"], out["y_ng"])


@pytest.mark.parametrize("cid", PROPERTY_CASES)
def test_batch_independence(oracle, products, cid):
    """Eval-mode BatchNorm does not couple the clouds: cloud 0 alone (B = 1, for sa1 and sa2 another kernel band than the batch) finds
    the same neighbours and gives row 0 of the batched output.  Both runs lie within GATE of the same float64 value (asserted for the
    batched one), hence the bound 2 GATE max|y64|; HIP against HIP on a continuous forward value, so no decision is injected there."""
    products.set_float32_products("split")
    module, (xyz, pts, centres, _), nbr, K, group_all, _ = _setup(cid, products)
    with torch.no_grad():
        y, routing = _tapped(lambda: _forward(cid, module, xyz, pts, centres, nbr, K, group_all))
        solo_nbr = None
        if nbr is not None:   # the radius query of the cloud alone
            xg = xyz[:1].cuda()
            solo_nbr = products.ball_query(FAMILY[cid[:2]][4], K, xg, products.index_points(xg, centres[:1].cuda()))
            assert torch.equal(solo_nbr, nbr[:1])
        y1, routing1 = _tapped(lambda: _forward(cid, module, xyz[:1], None if pts is None else pts[:1], None if group_all else centres[:1],
                                                solo_nbr, K, group_all))
    torch.cuda.synchronize()
    if not group_all:
        assert torch.equal(routing1["neighbours"][0], routing["neighbours"][0]), "the cloud alone found other neighbours"
    P = {"sa." + k.replace("mlp_", ""): v.detach().cpu().double() for k, v in module.state_dict().items() if v.is_floating_point()}
    _, y64, _ = oracle.sa_forward(xyz, None if pts is None else pts.double(), P, "sa", centres, None if group_all else K, group_all, False,
                                  oracle.BNState(), neighbour_idx=routing["neighbours"], argmax=routing["argmax"], relu_masks=routing["relu_masks"])
    scale = float(y64.abs().max())
    batched, solo = relmax(y, y64), float((y1[0] - y[0]).abs().max()) / scale
    print(f"\n[{cid}] batched against float64 {batched:.2e}; cloud 0 alone against row 0 of the batch {solo:.2e} (of max|y64| = {scale:.3g})")
    assert batched <= GATE
    assert solo <= 2 * GATE, solo
