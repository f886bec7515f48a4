// gemm_kernels.hip -- the grouped per-point MLP of PointNetSetAbstraction as fused GEMMs on the
// gfx950 matrix cores (reference: models/pointnet_pp_8dir.py:29-43 and its autograd backward).
//
// Arithmetic is exact float32: v_mfma_f32_32x32x2_f32 (one rounding per product, k-ordered fmaf
// chain; MI355X_MICROARCH "Matrix cores"), statistics are accumulated in float64.
//
// Layout: every activation tensor is row-major (rows = (cloud, centre, neighbour), channels
// contiguous), so a 1x1 Conv2d over (B,C,npoint,nsample) is C[M x N] = A[M x K] * W^T.
// What would be separate gather / concat / BatchNorm-apply / ReLU / BatchNorm-backward passes over
// HBM is folded into the A-operand loader of the consuming GEMM; column statistics, ReLU masks and
// the stores are folded into the epilogue of the producing GEMM.
//
// MFMA operand maps (wave64, 32x32x2 f32):  A: lane l holds A[i=l&31][k=l>>5]
//                                           B: lane l holds B[k=l>>5][j=l&31]
//                                           D: lane l, reg r: col j=l&31, row i=(r&3)+8*(r>>2)+4*(l>>5)
//
// This file: the generic chunked kernel, the small-M kernel (with the head's dx + dW launch, which runs the same 16-wave body), dZ
// materialisation and launch_gemm, the dispatcher -- the only place that orders the try_launch_* calls.  The A-operand loaders are in
// operand_load.h; the body of the small-M kernel, which da_dw_kernel (dw_kernels.hip) also runs, and the chunk constants KC / APITCH
// are in gemm_smallm.h.  The weights-stationary kernel is gemm_ws_kernels.hip, the dW family dw_kernels.hip, slab reductions /
// BatchNorm finalisation / pooling bn_pool_kernels.hip.
#include "gemm_smallm.h"
#include "launch.h"

namespace pnpp {

// A/B switch read once per process (PNPP_NO_MID=1: the group_all level stays on the 32 x 32 split-K kernels); the one reader, also
// asked by try_launch_da_dw (dw_kernels.hip)
bool mid_tiles_on() {
    static const bool on = env_int("PNPP_NO_MID", 0) == 0;
    return on;
}

// ---------------------------------------------------------------------------------------------
// fused GEMM: persistent row-tile workers (grid.x) x column tiles (grid.y)
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, int AMODE, int EMODE>
__global__ void __launch_bounds__(WM * WN * 64, 2)
gemm_kernel(const AOperand A, const BOperand B, int M, int Nout, int Kd, const Epilogue E) {
    constexpr int TM = BM / WM, TN = BN / WN, MT = TM / 32, NT = TN / 32;
    constexpr int NTHR = WM * WN * 64;
    static_assert(TM % 32 == 0 && TN % 32 == 0 && (BM * (KC / 4)) % NTHR == 0 && (KC * (BN / 4)) % NTHR == 0, "tile configuration");
    constexpr int BP = BN;
    __shared__ __attribute__((aligned(16))) float lds[BM * APITCH + KC * BP];
    float *As = lds, *Bs = lds + BM * APITCH;
    const float *__restrict__ Bm = B.b;
    const int ldb = B.ldb;
    const bool bvec = (ldb & 3) == 0 && ((uintptr_t)Bm & 15) == 0 && B.perm_D < 0;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int n0 = blockIdx.y * BN;

    double s1[NT], s2[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) s1[i] = s2[i] = 0.0;

    const int tiles = (M + BM - 1) / BM;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int m0 = tile * BM;
        f32x16 acc[MT][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        // software pipeline: chunk k0+KC is fetched into registers while chunk k0 is in the MFMA loop
        constexpr int NA = BM * (KC / 4) / NTHR, NB = KC * (BN / 4) / NTHR;
        RawA ra[NA];
        float4 rb[NB];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int f = tid + i * NTHR;
                ra[i] = fetch_a4<AMODE>(A, m0 + f / (KC / 4), k0 + 4 * (f % (KC / 4)), M, Kd);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int f = tid + i * NTHR;
                float t[4];
                if (!B.trans) {  // [k][n]: four consecutive n of one reduction row
                    const int kk = k0 + f / (BN / 4), n = n0 + 4 * (f % (BN / 4));
                    const float *src = Bm + (size_t)min(kk, B.rows - 1) * ldb;
                    if (bvec) {
                        const float4 v = *reinterpret_cast<const float4 *>(src + min(n, Nout - 4));
                        t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) t[e] = src[min(n + e, Nout - 1)];
                    }
                    const bool okk = kk < B.rows;
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] *= (okk && n + e < Nout) ? 1.f : 0.f;
                } else {  // [n][k]: four consecutive reduction indices of one output column; n runs fastest over the
                          // lanes so that the transposing LDS stores below are conflict-free
                    const int n = n0 + f % BN, kq = k0 + 4 * (f / BN);
                    const float *src = Bm + (size_t)min(n, Nout - 1) * ldb;
                    if (bvec) {
                        const float4 v = *reinterpret_cast<const float4 *>(src + min(kq, B.rows - 4));
                        t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int kp = min(kq + e, B.rows - 1);
                            int col = kp;
                            if (B.perm_D >= 0) col = kp < B.perm_D ? kp + 3 : kp - B.perm_D;
                            t[e] = src[col];
                        }
                    }
                    const bool okn = n < Nout;
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] *= (okn && kq + e < B.rows) ? 1.f : 0.f;
                }
                rb[i] = make_float4(t[0], t[1], t[2], t[3]);
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < Kd; k0 += KC) {
            __syncthreads();  // the previous chunk has been consumed
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int f = tid + i * NTHR;
                const int r = f / (KC / 4), q = f % (KC / 4);
                float v[4];
                xform_a4<AMODE>(A, ra[i], m0 + r, k0 + 4 * q, M, Kd, v);
                float *d = As + r * APITCH + 4 * q;
                d[0] = v[0], d[1] = v[1], d[2] = v[2], d[3] = v[3];
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int f = tid + i * NTHR;
                if (!B.trans) {
                    *reinterpret_cast<float4 *>(Bs + (f / (BN / 4)) * BP + 4 * (f % (BN / 4))) = rb[i];
                } else {
                    float *d = Bs + 4 * (f / BN) * BP + f % BN;
                    d[0] = rb[i].x, d[BP] = rb[i].y, d[2 * BP] = rb[i].z, d[3 * BP] = rb[i].w;
                }
            }
            __syncthreads();
            if (k0 + KC < Kd) fetch(k0 + KC);
            const int ksteps = min(KC, Kd - k0) >> 1;
            const float *ap = As + (wm * TM + l31) * APITCH + lh;
            const float *bp = Bs + lh * BP + wn * TN + l31;
            if (ksteps == KC / 2) {
#pragma unroll 4
                for (int s = 0; s < KC / 2; ++s) {
                    float a[MT], b[NT];
#pragma unroll
                    for (int i = 0; i < MT; ++i) a[i] = ap[i * 32 * APITCH + 2 * s];
#pragma unroll
                    for (int j = 0; j < NT; ++j) b[j] = bp[2 * s * BP + j * 32];
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
                }
            } else {
                for (int s = 0; s < ksteps; ++s) {
                    float a[MT], b[NT];
#pragma unroll
                    for (int i = 0; i < MT; ++i) a[i] = ap[i * 32 * APITCH + 2 * s];
#pragma unroll
                    for (int j = 0; j < NT; ++j) b[j] = bp[2 * s * BP + j * 32];
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
                }
            }
        }

        // epilogue: each register is one row; a half-wave writes 32 consecutive floats (128 B)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = n0 + wn * TN + j * 32 + l31;
                float sc = 0.f, sh = 0.f, mu = 0.f, is = 0.f;
                if constexpr (EMODE == E_MASK_STATS) {
                    if (col < Nout) sc = E.scale[col], sh = E.shift[col], mu = E.mu[col], is = E.istd[col];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const bool ok = row < M && col < Nout;
                    float v = ok ? acc[i][j][r] : 0.f;  // padding rows are exact zeros: they add nothing to the sums
                    if constexpr (EMODE == E_STORE_STATS) {
                        s1[j] += (double)v;
                        s2[j] += (double)v * (double)v;
                    } else if constexpr (EMODE == E_MASK_STATS) {
                        const float zp = E.zp[(size_t)min(row, M - 1) * E.ldc + min(col, Nout - 1)];
                        v = (fmaf(zp, sc, sh) > 0.f) ? v : 0.f;
                        s1[j] += (double)v;
                        s2[j] += (double)v * (double)((zp - mu) * is);
                    }
                    if (ok) E.c[(size_t)row * E.ldc + col] = v;
                }
            }
    }

    if constexpr (EMODE != E_STORE) {
        // column partials: two lane halves -> WM waves (through LDS) -> one slab row per block.x
        __syncthreads();
        double *red = reinterpret_cast<double *>(lds);  // [WM][2][BN]
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            double a = s1[j] + shfl_xor_f64(s1[j], 32);
            double b = s2[j] + shfl_xor_f64(s2[j], 32);
            if (lh == 0) {
                const int cl = wn * TN + j * 32 + l31;
                red[(wm * 2 + 0) * BN + cl] = a;
                red[(wm * 2 + 1) * BN + cl] = b;
            }
        }
        __syncthreads();
        for (int f = tid; f < 2 * BN; f += NTHR) {
            const int which = f / BN, cl = f % BN;
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < WM; ++w) t += red[(w * 2 + which) * BN + cl];
            if (n0 + cl < Nout) E.slab[((size_t)blockIdx.x * 2 + which) * Nout + n0 + cl] = t;
        }
    }
}

// small-M GEMM (fully connected head, group_all levels): one 32 x 32 output tile per workgroup, body in gemm_smallm.h
template <int AMODE, int EMODE, bool BT, int NW>
__global__ void __launch_bounds__(NW * 64)
gemm_smallm_kernel(const AOperand A, const BOperand B, int M, int Nout, int Kd, const Epilogue E) {
    gemm_smallm_body<AMODE, EMODE, BT, NW>(A, B, M, Nout, Kd, E, blockIdx.x, blockIdx.y, gridDim.x * gridDim.y);
}

template <int AM, int EM>
static void launch_smallm_t(const AOperand &A, const BOperand &B, int M, int Nout, int Kd, const Epilogue &E, dim3 grid,
                            hipStream_t st) {
    if constexpr (AM == A_PLAIN) {
        // one row of tiles (the head, M <= 32): few workgroups and a long reduction, so K is split over 16 waves -- two
        // 32-deep chunks per wave at K = 1024 instead of eight dependent load round trips
        if (grid.y == 1 && Kd >= 256) {
            if (B.trans) hipLaunchKernelGGL((gemm_smallm_kernel<AM, EM, true, 16>), grid, dim3(1024), 0, st, A, B, M, Nout, Kd, E);
            else hipLaunchKernelGGL((gemm_smallm_kernel<AM, EM, false, 16>), grid, dim3(1024), 0, st, A, B, M, Nout, Kd, E);
            return;
        }
    }
    if (B.trans) hipLaunchKernelGGL((gemm_smallm_kernel<AM, EM, true, 4>), grid, dim3(256), 0, st, A, B, M, Nout, Kd, E);
    else hipLaunchKernelGGL((gemm_smallm_kernel<AM, EM, false, 4>), grid, dim3(256), 0, st, A, B, M, Nout, Kd, E);
}
template <int AM>
static int launch_smallm_e(const AOperand &A, const BOperand &B, int M, int Nout, int Kd, const Epilogue &E, dim3 grid,
                           hipStream_t st) {
    switch (E.mode) {
        case E_STORE: launch_smallm_t<AM, E_STORE>(A, B, M, Nout, Kd, E, grid, st); return PNPP_OK;
        case E_STORE_STATS: launch_smallm_t<AM, E_STORE_STATS>(A, B, M, Nout, Kd, E, grid, st); return PNPP_OK;
        case E_MASK_STATS: launch_smallm_t<AM, E_MASK_STATS>(A, B, M, Nout, Kd, E, grid, st); return PNPP_OK;
        case E_BN_APPLY:
            if constexpr (AM == A_PLAIN) {
                PNPP_REQUIRE(grid.y == 1 && E.bn.mean && E.bn.istd && E.bn.scale && E.bn.shift && E.bn.y, PNPP_ERR_ARG,
                             "gemm(small M): the BatchNorm epilogue needs all rows in one tile (M <= 32) and its outputs");
                launch_smallm_t<AM, E_BN_APPLY>(A, B, M, Nout, Kd, E, grid, st);
                return PNPP_OK;
            }
            break;
    }
    set_error("gemm(small M): bad epilogue mode %d", E.mode);
    return PNPP_ERR_ARG;
}

template <int BM, int BN, int WM, int WN>
static int launch_gemm_cfg(const AOperand &A, const BOperand &B, int M, int Nout, int Kd, const Epilogue &E, int *nslab,
                           hipStream_t st) {
    const int tiles = cdiv(M, BM);
    const int gx = tiles < kMaxStatBlocks ? tiles : kMaxStatBlocks;
    const dim3 grid(gx, cdiv(Nout, BN)), block(WM * WN * 64);
    if (nslab) *nslab = gx;
    ProfScope ps(st, "gemm_kernel<%d,%d,%d,%d,A%d,E%d> M=%d N=%d K=%d grid=%dx%d", BM, BN, WM, WN, A.mode, E.mode, M, Nout, Kd,
                 grid.x, grid.y);
#define PNPP_LAUNCH(AM, EM)                                                                                   \
    hipLaunchKernelGGL((gemm_kernel<BM, BN, WM, WN, AM, EM>), grid, block, 0, st, A, B, M, Nout, Kd, E); \
    break;
#define PNPP_BY_E(AM)                                                          \
    switch (E.mode) {                                                          \
        case E_STORE: PNPP_LAUNCH(AM, E_STORE)                                 \
        case E_STORE_STATS: PNPP_LAUNCH(AM, E_STORE_STATS)                     \
        case E_MASK_STATS: PNPP_LAUNCH(AM, E_MASK_STATS)                       \
        default: set_error("gemm: bad epilogue mode %d", E.mode); return PNPP_ERR_ARG; \
    }                                                                          \
    break;
    switch (A.mode) {
        case A_PLAIN: PNPP_BY_E(A_PLAIN)
        case A_BNRELU: PNPP_BY_E(A_BNRELU)
        case A_GATHER: PNPP_BY_E(A_GATHER)
        case A_CONCAT: PNPP_BY_E(A_CONCAT)
        case A_DZ: PNPP_BY_E(A_DZ)
        case A_DZ_POOL: PNPP_BY_E(A_DZ_POOL)
        default: set_error("gemm: bad A mode %d", A.mode); return PNPP_ERR_ARG;
    }
#undef PNPP_BY_E
#undef PNPP_LAUNCH
    PNPP_CHECK_LAUNCH("gemm");
    return PNPP_OK;
}

// Epilogue::pool_ext is honoured by the interior epilogue of the float32 weights-stationary kernel with one column tile per wave
// (every dense launch of try_launch_ws); the caller asks before it relies on it
bool gemm_pools_in_epilogue(const AOperand &A, int M, int Nout, int Kd, int nsample) {
    if (nsample != 32) return false;
    if (M < 8192) return mid_tiles_on() && mid_gemm_pools(A, M, Nout, Kd);   // group_all levels of 32-point clouds: the 64 x 64 kernel
    if (matmul_precision() != 0) return false;
    if (M % 64 != 0 || Nout % 64 != 0) return false;
    if (!(A.mode == A_PLAIN || A.mode == A_BNRELU)) return false;
    if (A.lda % 4 != 0 || ((uintptr_t)A.a & 15) != 0) return false;
    return Kd == 64 || Kd == 128 || Kd == 256;
}

int launch_gemm(const AOperand &A, const BOperand &Bin, int M, int Nout, int Kd, const Epilogue &Ein, int *nslab,
                hipStream_t st, int *dw_slabs) {
    Epilogue E = Ein;
    E.store_policy = store_policy();
    if (dw_slabs) *dw_slabs = 0;
    PNPP_REQUIRE(M > 0 && Nout > 0 && Kd > 0, PNPP_ERR_ARG, "gemm: non-positive size M=%d N=%d K=%d", M, Nout, Kd);
    PNPP_REQUIRE(Bin.b && Bin.ldb > 0, PNPP_ERR_ARG, "gemm: null B operand");
    PNPP_REQUIRE(Kd % 4 == 0, PNPP_ERR_ARG, "gemm: K=%d must be a multiple of 4", Kd);
    BOperand B = Bin;
    if (B.rows <= 0 || B.rows > Kd) B.rows = Kd;
    {
        int rc = PNPP_OK;
        if (try_launch_ws_bf16(A, B, M, Nout, Kd, E, nslab, st, &rc, dw_slabs)) return rc;   // only in the opt-in bf16-operand mode
        if (try_launch_wsf3(A, B, M, Nout, Kd, E, nslab, st, &rc)) return rc;  // the same products from exact bf16 splits (gemm_wsf3_kernels.hip)
        if (try_launch_wsf(A, B, M, Nout, Kd, E, nslab, st, &rc)) return rc;   // forward products: wave-private strips
        if (try_launch_wsd3(A, B, M, Nout, Kd, E, nslab, st, &rc, dw_slabs)) return rc;  // fused backward products of the grouped levels, split products, wave pairs
        if (try_launch_wsp(A, B, M, Nout, Kd, E, nslab, st, &rc, dw_slabs)) return rc;   // fused backward products, 64-channel input
        if (try_launch_wsq(A, B, M, Nout, Kd, E, nslab, st, &rc, dw_slabs)) return rc;   // the same for the 256-channel last layer
        if (try_launch_ws(A, B, M, Nout, Kd, E, nslab, st, &rc, dw_slabs)) return rc;
        if (mid_tiles_on() && try_launch_mid_gemm(A, B, M, Nout, Kd, E, nslab, st, &rc)) return rc;
    }
    const bool a_aligned = (A.mode == A_CONCAT || A.mode == A_GATHER) || (A.lda % 4 == 0 && ((uintptr_t)A.a & 15) == 0);
    if (M <= 4096 && cdiv(M, 32) <= kMaxStatBlocks && a_aligned && A.mode != A_GATHER) {
        // split-K 32x32 tiles: the fully connected head (M = batch) and the group_all layers (M = B * 32)
        const dim3 grid(cdiv(Nout, 32), cdiv(M, 32));
        if (nslab) *nslab = grid.y;
        ProfScope ps(st, "gemm_smallm_kernel<A%d,E%d,T%d> M=%d N=%d K=%d grid=%dx%d", A.mode, E.mode, B.trans, M, Nout, Kd, grid.x,
                     grid.y);
        int rc = PNPP_OK;
        switch (A.mode) {
            case A_PLAIN: rc = launch_smallm_e<A_PLAIN>(A, B, M, Nout, Kd, E, grid, st); break;
            case A_BNRELU: rc = launch_smallm_e<A_BNRELU>(A, B, M, Nout, Kd, E, grid, st); break;
            case A_CONCAT: rc = launch_smallm_e<A_CONCAT>(A, B, M, Nout, Kd, E, grid, st); break;
            case A_DZ: rc = launch_smallm_e<A_DZ>(A, B, M, Nout, Kd, E, grid, st); break;
            case A_DZ_POOL: rc = launch_smallm_e<A_DZ_POOL>(A, B, M, Nout, Kd, E, grid, st); break;
            default: set_error("gemm(small M): bad A mode %d", A.mode); return PNPP_ERR_ARG;
        }
        if (rc != PNPP_OK) return rc;
        PNPP_CHECK_LAUNCH("gemm(small M)");
        return PNPP_OK;
    }
    if (A.mode == A_PLAIN || A.mode == A_BNRELU || A.mode == A_DZ || A.mode == A_DZ_POOL)
        PNPP_REQUIRE(A.lda % 4 == 0 && ((uintptr_t)A.a & 15) == 0, PNPP_ERR_ARG, "gemm: A operand pitch/alignment");
    // tile shape: tall tiles for the grouped layers (M = B*npoint*nsample), square-ish for small M
    if (M >= 128 * 128) {
        if (Nout % 128 == 0) return launch_gemm_cfg<128, 128, 4, 2>(A, B, M, Nout, Kd, E, nslab, st);
        if (Nout % 64 == 0) return launch_gemm_cfg<128, 64, 4, 2>(A, B, M, Nout, Kd, E, nslab, st);
        return launch_gemm_cfg<128, 32, 4, 1>(A, B, M, Nout, Kd, E, nslab, st);
    }
    if (M > 32) {
        if (Nout % 64 == 0) return launch_gemm_cfg<64, 64, 2, 2>(A, B, M, Nout, Kd, E, nslab, st);
        return launch_gemm_cfg<128, 32, 4, 1>(A, B, M, Nout, Kd, E, nslab, st);
    }
    if (Nout % 128 == 0) return launch_gemm_cfg<32, 128, 1, 4>(A, B, M, Nout, Kd, E, nslab, st);
    return launch_gemm_cfg<128, 32, 4, 1>(A, B, M, Nout, Kd, E, nslab, st);
}

// ---------------------------------------------------------------------------------------------
// small-M layers (group_all: M = 32 * B): the BatchNorm-backward operand dZ is materialised once (a few MB)
// instead of being rebuilt by every 32 x 32 output tile of the dA and dW GEMMs that consume it
// ---------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(256) dz_materialize_kernel(const AOperand A, int M, int C, float *__restrict__ out) {
    const size_t total = (size_t)M * (C / 4);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int row = (int)(i / (C / 4)), k = 4 * (int)(i % (C / 4));
        const RawA r = fetch_a4<MODE>(A, row, k, M, C);
        float v[4];
        xform_a4<MODE>(A, r, row, k, M, C, v);
        *reinterpret_cast<float4 *>(out + (size_t)row * C + k) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

int launch_dz_materialize(const AOperand &dz, int M, int C, float *out, hipStream_t st) {
    PNPP_REQUIRE(C % 4 == 0 && (dz.mode == A_DZ || dz.mode == A_DZ_POOL), PNPP_ERR_ARG, "dz_materialize: bad operand");
    const size_t total = (size_t)M * (C / 4);
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    ProfScope ps(st, "dz_materialize_kernel M=%d C=%d", M, C);
    if (dz.mode == A_DZ) hipLaunchKernelGGL(dz_materialize_kernel<A_DZ>, dim3(grid), dim3(256), 0, st, dz, M, C, out);
    else hipLaunchKernelGGL(dz_materialize_kernel<A_DZ_POOL>, dim3(grid), dim3(256), 0, st, dz, M, C, out);
    PNPP_CHECK_LAUNCH("dz_materialize");
    return PNPP_OK;
}

// The head layers (M <= 32 rows): dx = dz W as one row of 32 x 32 split-K tiles (16 waves) and dW = dz^T x as an outer
// product (no reduction worth an MFMA tile; workgroup = 32 output rows n x 128 columns k, dz and x tiles in LDS, each
// thread one k and four n) only share dz: one launch, the first g1 workgroups take the GEMM tiles.
__device__ __forceinline__ void dw_fewrows_body(const float *__restrict__ dz, const float *__restrict__ x, int M, int N, int K,
                                                float *__restrict__ dw, int bx, int by) {
    __shared__ __attribute__((aligned(16))) float dzs[32][32];
    __shared__ float xs[32][128];
    const int kl = threadIdx.x & 127, nh = threadIdx.x >> 7;  // 1024 threads: 8 groups of 4 output rows
    const int k0 = bx * 128, n0 = by * 32;
    for (int f = threadIdx.x; f < 32 * 32; f += 1024) {
        const int m = f >> 5, n = f & 31;
        dzs[m][n] = (m < M && n0 + n < N) ? dz[(size_t)m * N + n0 + n] : 0.f;
    }
    for (int f = threadIdx.x; f < 32 * 128; f += 1024) {
        const int m = f >> 7, k = f & 127;
        xs[m][k] = (m < M && k0 + k < K) ? x[(size_t)m * K + k0 + k] : 0.f;
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int m = 0; m < 32; ++m) {
        const float xv = xs[m][kl];
        const float4 d = *reinterpret_cast<const float4 *>(&dzs[m][4 * nh]);
        acc[0] = fmaf(d.x, xv, acc[0]), acc[1] = fmaf(d.y, xv, acc[1]);
        acc[2] = fmaf(d.z, xv, acc[2]), acc[3] = fmaf(d.w, xv, acc[3]);
    }
    if (k0 + kl < K)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + 4 * nh + j;
            if (n < N) dw[(size_t)n * K + k0 + kl] = acc[j];
        }
}

__global__ void __launch_bounds__(1024)
fc_dx_dw_kernel(const AOperand dzA, const BOperand W, int M, int Nout, int Kd, const Epilogue E, int g1, const float *__restrict__ x,
                int N, int K, int gx2, float *__restrict__ dw) {
    if ((int)blockIdx.x < g1) gemm_smallm_body<A_PLAIN, E_STORE, false, 16>(dzA, W, M, Nout, Kd, E, blockIdx.x, 0, g1);
    else dw_fewrows_body(dzA.a, x, M, N, K, dw, (blockIdx.x - g1) % gx2, (blockIdx.x - g1) / gx2);
}

// dz: (M, N) row-major with pitch N; W: (N, K) row-major; dx: (M, K); dw: (N, K).  false = not this form, nothing launched.
bool try_launch_fc_dx_dw(const float *dz, const float *w, const float *x, int M, int N, int K, float *dx, float *dw, hipStream_t st,
                         int *rc) {
    *rc = PNPP_OK;
    if (!(M <= 32 && N >= 256 && N % 4 == 0 && K % 4 == 0 && ((uintptr_t)dz & 15) == 0)) return false;
    AOperand A;
    A.a = dz;
    A.lda = N;
    BOperand B;
    B.b = w;
    B.ldb = K;
    B.rows = N;
    Epilogue E;
    E.mode = E_STORE;
    E.c = dx;
    E.ldc = K;
    const int g1 = cdiv(K, 32), gx2 = cdiv(K, 128), gy2 = cdiv(N, 32);
    ProfScope ps(st, "fc_dx_dw_kernel M=%d N=%d K=%d grid=%d+%d", M, N, K, g1, gx2 * gy2);
    hipLaunchKernelGGL(fc_dx_dw_kernel, dim3(g1 + gx2 * gy2), dim3(1024), 0, st, A, B, M, K, N, E, g1, x, N, K, gx2, dw);
    check_launch("fc_dx_dw", rc);
    return true;
}

}  // namespace pnpp
