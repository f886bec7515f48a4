// gemm_ws_kernels.hip -- the float32 weights-stationary GEMM of the grouped layers (gemm_ws_kernel) and its launch fan.  Layout and MFMA
// operand maps: the head of gemm_kernels.hip.  try_launch_ws is one of the try_launch_* forms launch_gemm (gemm_kernels.hip) orders.
#include "launch.h"

namespace pnpp {

// ---------------------------------------------------------------------------------------------
// weights-stationary GEMM for the grouped layers (M = B*npoint*nsample rows, K and N <= 260):
//   * the whole weight panel W[K x BN] is staged ONCE per workgroup and stays in LDS;
//   * a workgroup is a persistent worker over row tiles; per tile the whole A'[BM x K] panel is staged
//     in one shot (transform applied on the way in), so there are two barriers per tile instead of
//     two per 32-deep K chunk, and the next tile's HBM stream is already in flight (registers) while
//     the current tile runs its K/2 MFMA steps -- a full tile of compute hides the load latency;
//   * only the HBM streams are prefetched; L2-resident side tables (pooled gradient, arg-max,
//     per-channel constants) are read when the tile is written to LDS.
// Layout of the reduction dimension for grouped operands: [features (D) | x y z 0].
// ---------------------------------------------------------------------------------------------
struct RawTail {
    float x0, x1, x2, c0, c1, c2;
};

template <int MODE>
__device__ __forceinline__ RawTail ws_fetch_tail(const AOperand &A, int row, int M) {
    RawTail t{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (MODE == A_GATHER || MODE == A_CONCAT) {
        const int rc = min(row, M - 1);
        size_t prow = (size_t)rc;
        if constexpr (MODE == A_GATHER) {
            const size_t grp = (size_t)(rc / A.K);
            prow = (size_t)(grp / A.S) * A.N + A.idx[rc];
            const float *cp = A.new_xyz + grp * 3;
            t.c0 = cp[0], t.c1 = cp[1], t.c2 = cp[2];
        }
        const float *xp = A.xyz + prow * 3;
        t.x0 = xp[0], t.x1 = xp[1], t.x2 = xp[2];
    }
    return t;
}

#ifdef PNPP_STAMPS
__device__ unsigned long long g_stamps[16];
__device__ int g_stamp_kd;
#define PNPP_STAMP(i)                                                 \
    if (st_on) {                                                      \
        __builtin_amdgcn_s_waitcnt(0);                                \
        const unsigned long long st_t = __builtin_amdgcn_s_memtime(); \
        if (lane == 0) g_stamps[i] += st_t - st_last;                 \
        st_last = st_t;                                               \
    }
#else
#define PNPP_STAMP(i)
#endif
// timing experiments only (results are WRONG with either on; never in a shipped build): what is left of a launch without its
// matrix instructions, or without its output stores
#ifndef PNPP_WS_EXP_NO_MFMA
#define PNPP_WS_EXP_NO_MFMA 0
#endif
#ifndef PNPP_WS_EXP_NO_STORE
#define PNPP_WS_EXP_NO_STORE 0
#endif
#if PNPP_WS_EXP_NO_MFMA
#define PNPP_WS_MFMA(a, b, c) ((c)[0] += (a) + (b), (c))
#else
#define PNPP_WS_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#endif

// KD: reduction length (compile time; for grouped operands KD = D + 4 with the [x y z 0] tail last).
// Thread -> (column group kq = tid % G4, rows tid / G4 + i * RPP): every thread keeps ONE column group
// for the whole kernel, so its per-channel constants live in registers, and with K_nbr == 32 the
// pooled-gradient / arg-max entries of a tile's few neighbour groups are fetched once per tile.
template <int KD, int BM, int BN, int WM, int WN, int AMODE, int EMODE, bool FDW>
__global__ void __launch_bounds__(256, (KD >= 256 ? 1 : 2))  // the K=256 panels leave room for one workgroup per CU anyway
gemm_ws_kernel(const AOperand A, const BOperand B, int M, int Nout, int ncol, const Epilogue E) {
    constexpr int TM = BM / WM, TN = BN / WN, MT = TM / 32, NT = TN / 32;
    constexpr bool ONE_WAVE = KD >= 256;   // one wave per SIMD (the launch bounds above): registers to spare, and every VALU is MFMA time
    constexpr bool HAS_TAIL = (AMODE == A_GATHER || AMODE == A_CONCAT);
    constexpr int KMAIN = HAS_TAIL ? KD - 4 : KD;  // columns served by the float4 stream
    constexpr int G4 = KMAIN / 4;                  // column groups per row
    constexpr int RPP = G4 > 0 ? 256 / (G4 > 0 ? G4 : 1) : 1;  // rows staged per pass
    constexpr int NG = G4 > 0 ? BM / RPP : 0;      // passes per tile
    // A tile addressing: element (r, k) lives at r*KP + (k ^ f(r)), f(r) = (r & 15) << 2, when KD is a multiple of 64:
    // an XOR swizzle of whole 16-byte groups, no padding.  The dA operand is read lane-per-row as ONE ds_read_b128 per
    // four MFMA steps (the 16-lane groups of that instruction hold rows that are distinct mod 16, so they land on 16
    // different groups of a 256-byte bank row); the dW operand is read lane-per-column with ds_read_b32 (fixed r: the
    // XOR permutes an aligned block of 32 columns, 32 different banks); a staged float4 is one ds_write_b128 of the
    // registers as loaded.  The weight tile uses the same image, [n][k ^ f(n)].  Otherwise (KD = D + 4) element
    // (r, k) is at r*(KD+1) + k and the weights are [k][n].
    constexpr bool SWZ = (KD % 64 == 0);
    constexpr int KP = SWZ ? KD : KD + 1;
    constexpr int GPT = (BM + 31) / 32;            // neighbour groups per tile when nsample == 32
    constexpr int DW_TILES = FDW ? (KD / 32) * (BN / 32) : 0, DT = FDW ? (DW_TILES + 3) / 4 : 1;
    static_assert(!FDW || (EMODE == E_MASK_STATS && SWZ && DW_TILES % 4 == 0), "fused dW needs the ReLU-mask epilogue");
    static_assert(!FDW || NT == 1, "fused dW exists on the 64 x 64 / 2 x 2 tiles only: one column tile per wave");
    static_assert(WM * WN == 4 && TM % 32 == 0 && TN % 32 == 0, "tile configuration");
    static_assert(G4 == 0 || (256 % G4 == 0 && BM % RPP == 0 && (32 % RPP == 0 || RPP % 32 == 0)), "staging map");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Ws = lds;            // [KD][BN], or [BN][KD] swizzled (SWZ)
    float *As = lds + KD * BN;  // [BM][KP]
    float *Ap = As + BM * KP;   // FDW: [BM][BN] = relu(bn(zp)) tile, the dW GEMM's second operand
    auto a_swz = [](int r) { return (r & 15) << 2; };
    auto a_idx = [&](int r, int k) { return r * KP + (SWZ ? (k ^ a_swz(r)) : k); };

    // the wave index is uniform: telling the compiler so moves the tile-row / tile-column arithmetic of every address to the scalar unit
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
#ifdef PNPP_STAMPS
    // selector: KD for the fused pooled backward kernels, 1000 + KD for the forward kernels (BN+ReLU operand, statistics)
    const bool st_on = blockIdx.x == 8 && wave == 0 &&
                       ((FDW && AMODE == A_DZ_POOL && g_stamp_kd == KD) ||
                        (!FDW && AMODE == A_BNRELU && EMODE == E_STORE_STATS && g_stamp_kd == 1000 + KD));
    unsigned long long st_last = __builtin_amdgcn_s_memtime();
#endif
    // XCD-aware tile map (speed only, never correctness): blocks b and b + 8 share an XCD and with it an L2, so the ncol
    // column blocks of one worker -- which stream the SAME operand rows -- are placed 8 apart: the rows come from HBM once
    // and from that L2 for the other column blocks, instead of once per XCD
    const int nworkers = gridDim.x / ncol;
    int col_blk = blockIdx.x % ncol, worker = blockIdx.x / ncol;
    if ((nworkers & 7) == 0) {
        const int xcd = blockIdx.x & 7, i = blockIdx.x >> 3;
        col_blk = i % ncol, worker = (i / ncol) * 8 + xcd;
    }
    const int n0 = col_blk * BN;
    const int kq = G4 > 0 ? 4 * (tid % (G4 > 0 ? G4 : 1)) : 0;  // this thread's first column
    const int r_base = G4 > 0 ? tid / (G4 > 0 ? G4 : 1) : 0;

    // ---- per-channel constants of this thread's column group: registers for the whole kernel.  Their loads go out FIRST (the table
    // was written by the previous launch: a cold ~1.5 us round trip), then the weight panel's, then the first tile's: one wait
    // covers the three instead of three round trips in a row ----
    float4 c_g = make_float4(0.f, 0.f, 0.f, 0.f), c_mu = c_g, c_is = c_g, c_c1 = c_g, c_c2 = c_g, c_sc = c_g, c_sh = c_g;
    if constexpr (G4 > 0 && (AMODE == A_DZ || AMODE == A_DZ_POOL)) {
        const float *c = A.cst + kq;
        c_g = *reinterpret_cast<const float4 *>(c);
        c_mu = *reinterpret_cast<const float4 *>(c + A.C);
        c_is = *reinterpret_cast<const float4 *>(c + 2 * A.C);
        c_c1 = *reinterpret_cast<const float4 *>(c + 3 * A.C);
        c_c2 = *reinterpret_cast<const float4 *>(c + 4 * A.C);
    } else if constexpr (G4 > 0 && AMODE == A_BNRELU) {
        c_sc = *reinterpret_cast<const float4 *>(A.scale + kq);
        c_sh = *reinterpret_cast<const float4 *>(A.shift + kq);
    }

    const int tiles = (M + BM - 1) / BM;
    const bool pool_fast = (AMODE == A_DZ_POOL) && A.K == 32;  // tiles start on neighbour-group boundaries (BM % 32 == 0)
    float4 rp[NG > 0 ? NG : 1], rq[(AMODE == A_DZ && NG > 0) ? NG : 1];
    RawTail rt;
    // M a multiple of BM (every shape of the training step): no row of a tile needs a clamp or a bounds test, and the operand
    // streams are (uniform tile pointer, advanced by scalar arithmetic) + (one 32-bit lane offset computed once) -- the 64-bit
    // multiply-add, clamp and EXEC branch per 16-byte group were a third of the staging pass, and VALU time is MFMA time
    // (measured: -4.6 % on the K = 256 kernels, which run one wave per SIMD; nothing or a small loss on the K <= 128 kernels with
    // two waves per SIMD, which keep the general path)
    // (round 3 A/B, two traces per variant on one box: for K <= 128 the clamp-free pass alone is +1.4 / +2.2 us on the pooled K = 128
    // and the K = 64 backward launch; together with the dW address table it is -2.4 us on the pooled K = 128 launch and 0 / +0.3
    // on the others -- so that one instantiation takes both)
    constexpr bool TUNED_128 = KD == 128 && AMODE == A_DZ_POOL && FDW;
    constexpr bool DENSE_A = (AMODE == A_PLAIN || AMODE == A_BNRELU || AMODE == A_DZ || AMODE == A_DZ_POOL) && (ONE_WAVE || TUNED_128);
    const bool full_rows = DENSE_A && (M % BM) == 0 && (AMODE != A_DZ_POOL || A.K == 32);
    const unsigned offA = (unsigned)r_base * (unsigned)A.lda + (unsigned)kq;
    auto fetch = [&](int m0) {
        if constexpr (DENSE_A) {
            if (full_rows) {
                const float *pa = (AMODE == A_DZ_POOL ? A.z : A.a) + (size_t)m0 * A.lda;
                const float *pz = A.z + (size_t)m0 * A.lda;
#pragma unroll
                for (int i = 0; i < NG; ++i) {
                    rp[i] = *reinterpret_cast<const float4 *>(pa + (size_t)(i * RPP) * A.lda + offA);
                    if constexpr (AMODE == A_DZ) rq[i] = *reinterpret_cast<const float4 *>(pz + (size_t)(i * RPP) * A.lda + offA);
                }
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int rc = min(m0 + r_base + i * RPP, M - 1);
            if constexpr (AMODE == A_PLAIN || AMODE == A_BNRELU) {
                rp[i] = *reinterpret_cast<const float4 *>(A.a + (size_t)rc * A.lda + kq);
            } else if constexpr (AMODE == A_DZ) {
                rp[i] = *reinterpret_cast<const float4 *>(A.a + (size_t)rc * A.lda + kq);
                rq[i] = *reinterpret_cast<const float4 *>(A.z + (size_t)rc * A.lda + kq);
            } else if constexpr (AMODE == A_DZ_POOL) {
                rp[i] = *reinterpret_cast<const float4 *>(A.z + (size_t)rc * A.lda + kq);  // the only HBM stream
            } else if constexpr (AMODE == A_GATHER) {
                const size_t prow = (size_t)((rc / A.K) / A.S) * A.N + A.idx[rc];
                rp[i] = *reinterpret_cast<const float4 *>(A.a + prow * A.D + kq);
            } else {
                rp[i] = *reinterpret_cast<const float4 *>(A.a + (size_t)rc * A.D + kq);
            }
        }
        if constexpr (HAS_TAIL) rt = ws_fetch_tail<AMODE>(A, m0 + min(tid, BM - 1), M);
    };
    // vmcnt counts loads and stores in issue order on gfx9: a wait for a load issued AFTER a tile's 16 output stores is a wait
    // for those stores' acknowledgements too.  Everything the next staging pass reads is therefore requested before them.
    float4 gdm[GPT];
    int4 garg[GPT];
    auto fetch_pool = [&](int m0) {
        if constexpr (AMODE == A_DZ_POOL) {
            if (full_rows) {
#pragma unroll
                for (int g = 0; g < GPT; ++g) {
                    const size_t gi = (size_t)(m0 / 32 + g) * A.lda + kq;
                    gdm[g] = *reinterpret_cast<const float4 *>(A.a + gi);
                    garg[g] = *reinterpret_cast<const int4 *>(A.arg + gi);
                }
            } else if (pool_fast) {
#pragma unroll
                for (int g = 0; g < GPT; ++g) {
                    const size_t gi = (size_t)min(m0 / 32 + g, (M - 1) / 32) * A.lda + kq;
                    gdm[g] = *reinterpret_cast<const float4 *>(A.a + gi);
                    garg[g] = *reinterpret_cast<const int4 *>(A.arg + gi);
                }
            }
        }
    };
    int tile = worker;
    bool fetched = false;
    // ---- weights: staged once, [k][n] ----
    {
        const float *__restrict__ Bm = B.b;
        const int ldb = B.ldb;
        const bool bvec = (ldb & 3) == 0 && ((uintptr_t)Bm & 15) == 0 && B.perm_D < 0;
        // two passes: every 16-byte group of the panel this thread owns is REQUESTED first (all loads in flight together: one
        // L2 / HBM round trip for the whole panel instead of one per group of a rolled loop), then masked and written to LDS
        auto wload = [&](int f, float (&t)[4]) {
            if (!B.trans && SWZ) {
                // row-major panel -> [n][k ^ f(n)] image: lane = column (four dword loads of consecutive rows, each 256 B per
                // wave), then ONE conflict-free ds_write_b128 per group.  (The first version read 16 bytes along n and wrote
                // four transposed ds_write_b32 that met 8-way bank conflicts: 5.8 us of a 54 us launch went into this panel.)
                const int nl = f % BN, k4 = 4 * (f / BN), n = min(n0 + nl, Nout - 1);
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = Bm[(size_t)min(k4 + e, B.rows - 1) * ldb + n];
            } else if (!B.trans) {
                const int kk = f / (BN / 4), n = n0 + 4 * (f % (BN / 4));
                const float *src = Bm + (size_t)min(kk, B.rows - 1) * ldb;
                if (bvec) {
                    const float4 v = *reinterpret_cast<const float4 *>(src + min(n, Nout - 4));
                    t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = src[min(n + e, Nout - 1)];
                }
            } else {
                // swizzled image: consecutive lanes take consecutive 16-byte groups of ONE weight row (coalesced 1 KB per wave, and
                // the ds_write_b128 of a row land in distinct slots); the [k][n] image keeps lane = column
                const int nl = SWZ ? f / (KD / 4) : f % BN, k4 = SWZ ? 4 * (f % (KD / 4)) : 4 * (f / BN), n = n0 + nl;
                const float *src = Bm + (size_t)min(n, Nout - 1) * ldb;
                if (bvec) {
                    const float4 v = *reinterpret_cast<const float4 *>(src + min(k4, B.rows - 4));
                    t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int kp = min(k4 + e, B.rows - 1);
                        int col = kp;
                        if (B.perm_D >= 0) col = kp < B.perm_D ? kp + 3 : kp - B.perm_D;
                        t[e] = src[col];
                    }
                }
            }
        };
        auto wstore = [&](int f, float (&t)[4]) {
            if (!B.trans && SWZ) {
                const int nl = f % BN, k4 = 4 * (f / BN);
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] *= (n0 + nl < Nout && k4 + e < B.rows) ? 1.f : 0.f;
                *reinterpret_cast<float4 *>(Ws + nl * KD + (k4 ^ a_swz(nl))) = make_float4(t[0], t[1], t[2], t[3]);
            } else if (!B.trans) {
                const int kk = f / (BN / 4), n = n0 + 4 * (f % (BN / 4));
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] *= (kk < B.rows && n + e < Nout) ? 1.f : 0.f;
                if constexpr (SWZ) {  // transposed image: four scalar stores (once per workgroup)
                    const int nl = 4 * (f % (BN / 4));
#pragma unroll
                    for (int e = 0; e < 4; ++e) Ws[(nl + e) * KD + (kk ^ a_swz(nl + e))] = t[e];
                } else {
                    *reinterpret_cast<float4 *>(Ws + kk * BN + 4 * (f % (BN / 4))) = make_float4(t[0], t[1], t[2], t[3]);
                }
            } else {
                // swizzled image: consecutive lanes take consecutive 16-byte groups of ONE weight row (coalesced 1 KB per wave, and
                // the ds_write_b128 of a row land in distinct slots); the [k][n] image keeps lane = column
                const int nl = SWZ ? f / (KD / 4) : f % BN, k4 = SWZ ? 4 * (f % (KD / 4)) : 4 * (f / BN), n = n0 + nl;
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] *= (n < Nout && k4 + e < B.rows) ? 1.f : 0.f;
                if constexpr (SWZ) {
                    *reinterpret_cast<float4 *>(Ws + nl * KD + (k4 ^ a_swz(nl))) = make_float4(t[0], t[1], t[2], t[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) Ws[(k4 + e) * BN + nl] = t[e];
                }
            }
        };
        // (row-major panels of the backward kernels; for the [n][k] weights of the forward kernels the same two passes were worth
        // 0.2 us per launch and cost the backward instantiations as much -- A/B on one box, tools/ab_trace.sh -- so they keep the loop)
        constexpr int NWF = (KD * (BN / 4)) / 256;
        bool staged = false;
        if constexpr (SWZ && (KD * (BN / 4)) % 256 == 0 && NWF >= 4 && NWF <= 16) {
            if (!B.trans) {
                staged = true;
                float tw[NWF][4];
#pragma unroll
                for (int j = 0; j < NWF; ++j) wload(tid + 256 * j, tw[j]);
                if (tile < tiles) fetch(tile * BM);   // behind the panel in the queue: its HBM round trip overlaps the LDS writes
                fetched = true;
#pragma unroll
                for (int j = 0; j < NWF; ++j) wstore(tid + 256 * j, tw[j]);
            }
        }
        if (!staged) {
            for (int f = tid; f < KD * (BN / 4); f += 256) {
                float t[4];
                if (!B.trans) {
                    const int kk = f / (BN / 4), n = n0 + 4 * (f % (BN / 4));
                    const float *src = Bm + (size_t)min(kk, B.rows - 1) * ldb;
                    if (bvec) {
                        const float4 v = *reinterpret_cast<const float4 *>(src + min(n, Nout - 4));
                        t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
                    } else {
    #pragma unroll
                        for (int e = 0; e < 4; ++e) t[e] = src[min(n + e, Nout - 1)];
                    }
    #pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] *= (kk < B.rows && n + e < Nout) ? 1.f : 0.f;
                    if constexpr (SWZ) {  // transposed image: four scalar stores (once per workgroup)
                        const int nl = 4 * (f % (BN / 4));
    #pragma unroll
                        for (int e = 0; e < 4; ++e) Ws[(nl + e) * KD + (kk ^ a_swz(nl + e))] = t[e];
                    } else {
                        *reinterpret_cast<float4 *>(Ws + kk * BN + 4 * (f % (BN / 4))) = make_float4(t[0], t[1], t[2], t[3]);
                    }
                } else {
                    // swizzled image: consecutive lanes take consecutive 16-byte groups of ONE weight row (coalesced 1 KB per wave, and
                // the ds_write_b128 of a row land in distinct slots); the [k][n] image keeps lane = column
                const int nl = SWZ ? f / (KD / 4) : f % BN, k4 = SWZ ? 4 * (f % (KD / 4)) : 4 * (f / BN), n = n0 + nl;
                    const float *src = Bm + (size_t)min(n, Nout - 1) * ldb;
                    if (bvec) {
                        const float4 v = *reinterpret_cast<const float4 *>(src + min(k4, B.rows - 4));
                        t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
                    } else {
    #pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int kp = min(k4 + e, B.rows - 1);
                            int col = kp;
                            if (B.perm_D >= 0) col = kp < B.perm_D ? kp + 3 : kp - B.perm_D;
                            t[e] = src[col];
                        }
                    }
    #pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] *= (n < Nout && k4 + e < B.rows) ? 1.f : 0.f;
                    if constexpr (SWZ) {
                        *reinterpret_cast<float4 *>(Ws + nl * KD + (k4 ^ a_swz(nl))) = make_float4(t[0], t[1], t[2], t[3]);
                    } else {
    #pragma unroll
                        for (int e = 0; e < 4; ++e) Ws[(k4 + e) * BN + nl] = t[e];
                    }
                }
            }
        }
    }

    PNPP_STAMP(11)  // prologue: weight panel in LDS
    if (!fetched && tile < tiles) fetch(tile * BM);
    if (tile < tiles) fetch_pool(tile * BM);
    if constexpr (G4 > 0 && (AMODE == A_DZ || AMODE == A_DZ_POOL)) {
        // dz = g (dy - c1 - (z - mu) istd c2) as two FMAs per element: g dy + (a z + b), a = -g istd c2, b = -g c1 - a mu
        // (c_is keeps a, c_c1 keeps b from here on; six dependent VALU per element otherwise, and VALU time is MFMA time)
        c_is = make_float4(-c_g.x * c_is.x * c_c2.x, -c_g.y * c_is.y * c_c2.y, -c_g.z * c_is.z * c_c2.z, -c_g.w * c_is.w * c_c2.w);
        c_c1 = make_float4(-c_g.x * c_c1.x - c_is.x * c_mu.x, -c_g.y * c_c1.y - c_is.y * c_mu.y, -c_g.z * c_c1.z - c_is.z * c_mu.z,
                           -c_g.w * c_c1.w - c_is.w * c_mu.w);
    }

    PNPP_STAMP(12)  // prologue: per-channel constants
    double s1[NT], s2[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) s1[i] = s2[i] = 0.0;
    float pool_sg[NT];   // sign of gamma at this lane's columns (pooling in the epilogue: max z or min z)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        pool_sg[j] = 1.f;
        if constexpr (EMODE == E_STORE_STATS) {
            if (E.pool_ext && E.pool_gamma) pool_sg[j] = E.pool_gamma[min(n0 + wn * TN + j * 32 + l31, Nout - 1)] >= 0.f ? 1.f : -1.f;
        }
    }

    f32x16 dwacc[DT];  // FDW: this wave's (32 x 32) tiles of dW, accumulated over every row tile of the worker
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dwacc[t][r] = 0.f;

    // Forward kernels (one 32 x 32 tile per wave): the tile's output stores are DEFERRED to the next iteration, behind the staging
    // pass.  vmcnt counts loads and stores in issue order, and the compiler cannot prove how many stores separate the next tile's
    // operand loads from the wait in front of the staging pass (the first iteration has none), so it waits with vmcnt(0): every
    // tile then also waits for its predecessor's 16 stores to be ACKNOWLEDGED -- 3 to 6 us per forward launch (a build with the
    // stores compiled out: 30.0 -> 24.0, 19.4 -> 16.0, 23.7 -> 20.8 us).  Held back until the loads have been consumed, the
    // stores have a whole tile to drain before anything waits again.
    constexpr bool DEFER = EMODE != E_MASK_STATS && !FDW && MT == 1 && NT == 1;
    f32x16 held;
    float held_ext = 0.f;
    int held_arg = 0, held_m0 = -1;
    auto flush_held = [&]() {
        if constexpr (DEFER) {
            if (held_m0 >= 0) {
                if constexpr (EMODE == E_STORE_STATS) {
                    if (E.pool_ext && lh == 0) {
                        const size_t gi = (size_t)((held_m0 + wm * TM) >> 5) * E.ldc + (n0 + wn * TN + l31);
                        E.pool_ext[gi] = held_ext;
                        E.pool_arg[gi] = held_arg;
                    }
                }
                float *tb = E.c + (size_t)(held_m0 + wm * TM) * E.ldc + (n0 + wn * TN);
                const unsigned lo = (unsigned)(4 * lh) * (unsigned)E.ldc + (unsigned)l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) tb[(size_t)((r & 3) + 8 * (r >> 2)) * E.ldc + lo] = held[r];
                held_m0 = -1;
            }
        }
    };

    // see the K loop: with `inter` the operand loads of the NEXT tile are issued between this tile's MFMAs
    const bool inter = DENSE_A && ONE_WAVE && SWZ && EMODE == E_MASK_STATS && full_rows && n0 + BN <= Nout;
    PNPP_STAMP(8)   // prologue, rest: first tile's loads complete
    for (; tile < tiles; tile += nworkers) {
        const int m0 = tile * BM;
        PNPP_STAMP(0)
        // pooled gradient / arg-max of the tile's neighbour groups at this thread's columns (L2-resident tables): requested one
        // tile ahead (fetch_pool below), so that no load the staging pass waits for is YOUNGER than the previous tile's stores
        __syncthreads();  // previous tile's operand reads are done (and, first time, the weights are staged)
        PNPP_STAMP(1)
        // two copies of the staging pass, the compile-time flag FULL picking which one runs (full_rows is uniform): the copy for
        // M % BM == 0 has no bounds test, no zero fill and no EXEC branch per 16-byte group
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
        const bool FULL = pass == 0;
        if (FULL != full_rows) continue;
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int r = r_base + i * RPP, row = m0 + r;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (FULL || row < M) {
                if constexpr (AMODE == A_PLAIN || AMODE == A_GATHER || AMODE == A_CONCAT) {
                    v[0] = rp[i].x, v[1] = rp[i].y, v[2] = rp[i].z, v[3] = rp[i].w;
                } else if constexpr (AMODE == A_BNRELU) {
                    v[0] = fmaxf(fmaf(rp[i].x, c_sc.x, c_sh.x), 0.f);
                    v[1] = fmaxf(fmaf(rp[i].y, c_sc.y, c_sh.y), 0.f);
                    v[2] = fmaxf(fmaf(rp[i].z, c_sc.z, c_sh.z), 0.f);
                    v[3] = fmaxf(fmaf(rp[i].w, c_sc.w, c_sh.w), 0.f);
                } else {
                    float4 dy, z;
                    if constexpr (AMODE == A_DZ) {
                        dy = rp[i], z = rq[i];
                    } else {
                        z = rp[i];
                        float4 dm;
                        int4 ia;
                        int kk;
                        if (FULL || pool_fast) {   // (FULL implies pool_fast: no merge with the general path below)
                            // neighbour group of this row inside the tile: a constant per unrolled pass when RPP | 32
                            const int g = (RPP >= 32) ? r / 32 : (i * RPP) / 32;
                            dm = gdm[0], ia = garg[0];
#pragma unroll
                            for (int gg = 1; gg < GPT; ++gg)
                                if (g == gg) dm = gdm[gg], ia = garg[gg];
                            kk = r - g * 32;
                        } else {
                            const int g = row / A.K;
                            kk = row - g * A.K;
                            dm = *reinterpret_cast<const float4 *>(A.a + (size_t)g * A.lda + kq);
                            ia = *reinterpret_cast<const int4 *>(A.arg + (size_t)g * A.lda + kq);
                        }
                        dy.x = kk == ia.x ? dm.x : 0.f, dy.y = kk == ia.y ? dm.y : 0.f;
                        dy.z = kk == ia.z ? dm.z : 0.f, dy.w = kk == ia.w ? dm.w : 0.f;
                    }
                    v[0] = fmaf(c_g.x, dy.x, fmaf(c_is.x, z.x, c_c1.x));
                    v[1] = fmaf(c_g.y, dy.y, fmaf(c_is.y, z.y, c_c1.y));
                    v[2] = fmaf(c_g.z, dy.z, fmaf(c_is.z, z.z, c_c1.z));
                    v[3] = fmaf(c_g.w, dy.w, fmaf(c_is.w, z.w, c_c1.w));
                }
            }
            if constexpr (SWZ) {
                *reinterpret_cast<float4 *>(As + r * KP + (kq ^ a_swz(r))) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) As[a_idx(r, kq + e)] = v[e];
            }
        }
        }
        if constexpr (HAS_TAIL) {
            if (tid < BM) {
                const bool ok = m0 + tid < M;
                // [x-cx, y-cy, z-cz, 0]: float32 subtraction, pointnet_pp_8dir.py:32
                As[a_idx(tid, KMAIN + 0)] = ok ? __fsub_rn(rt.x0, rt.c0) : 0.f;
                As[a_idx(tid, KMAIN + 1)] = ok ? __fsub_rn(rt.x1, rt.c1) : 0.f;
                As[a_idx(tid, KMAIN + 2)] = ok ? __fsub_rn(rt.x2, rt.c2) : 0.f;
                As[a_idx(tid, KMAIN + 3)] = 0.f;
            }
        }
        flush_held();   // the previous tile's output: this tile's operand loads have just been consumed
        PNPP_STAMP(2)
        __syncthreads();
        PNPP_STAMP(3)
        // K >= 256 (one wave per SIMD), dense operand, full tiles: the next tile's operand loads and this tile's epilogue operand are
        // issued BETWEEN the MFMAs of the unrolled K loop below -- a memory instruction issues while the matrix pipe works
        // on the previous MFMA, whereas 32 loads issued in front of the loop are ~1k cycles in which the pipe idles
        const bool have_next = tile + nworkers < tiles;
        if (!inter && have_next) fetch((tile + nworkers) * BM);  // next tile's HBM stream flies during the MFMA loop
        if (have_next) fetch_pool((tile + nworkers) * BM);   // (this tile's entries were consumed by the staging pass above)

        // the ReLU-mask operand of the epilogue is fetched now and lands while the MFMA loop runs
        float zp[MT][NT][16];
        if constexpr (EMODE == E_MASK_STATS) {
          if (inter) {
            // (issued inside the K loop)
          } else if (full_rows && n0 + BN <= Nout) {
            const float *pzp = E.zp + (size_t)m0 * E.ldc;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const unsigned oz = (unsigned)(wm * TM + i * 32 + 4 * lh) * (unsigned)E.ldc + (unsigned)(n0 + wn * TN + j * 32 + l31);
#pragma unroll
                    for (int r = 0; r < 16; ++r) zp[i][j][r] = pzp[(size_t)((r & 3) + 8 * (r >> 2)) * E.ldc + oz];
                }
          } else {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int cc = min(n0 + wn * TN + j * 32 + l31, Nout - 1);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        zp[i][j][r] = E.zp[(size_t)min(row, M - 1) * E.ldc + cc];
                    }
                }
          }
        }

        f32x16 acc[MT][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        const float *bp = Ws + lh * BN + wn * TN + l31;
        if constexpr (SWZ) {
            // K loop for the swizzled tiles.  Lane (l31, lh) fetches the four reduction indices k = 64 c + 8 t + 4 lh + {0..3}
            // of its row (A) and of its column (W) with one ds_read_b128 each and feeds them to four MFMA steps -- both
            // operands of a step carry the same k for the same lh, which is all the instruction asks for.  The swizzled
            // group is 64 c + ((8 t) ^ (4 lh ^ f)), so for a fixed t the NC = KD / 64 reads of a lane differ by an immediate
            // offset only: one xor + one add of address arithmetic per operand and t (an fp32 MFMA and VALU work of the
            // same SIMD do not overlap, so every VALU in this loop is MFMA time lost).  t is the rolled, software-pipelined
            // loop (reads of t + 1 are issued before the MFMAs of t); c is unrolled.
            constexpr int NC = KD / 64;
            const float *arow[MT], *brow[NT];
            int ga[MT], gb[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int r = wm * TM + i * 32 + l31;
                arow[i] = As + r * KP;
                ga[i] = (4 * lh) ^ a_swz(r);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = wn * TN + j * 32 + l31;
                brow[j] = Ws + n * KD;
                gb[j] = (4 * lh) ^ a_swz(n);
            }
            float4 ra[2][NC][MT], rb[2][NC][NT];
            auto ld = [&](int buf, int t) {
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const float *pa = arow[i] + ((8 * t) ^ ga[i]);
#pragma unroll
                    for (int c = 0; c < NC; ++c) ra[buf][c][i] = *reinterpret_cast<const float4 *>(pa + 64 * c);
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const float *pb = brow[j] + ((8 * t) ^ gb[j]);
#pragma unroll
                    for (int c = 0; c < NC; ++c) rb[buf][c][j] = *reinterpret_cast<const float4 *>(pb + 64 * c);
                }
            };
            auto mm = [&](int buf) {
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            acc[i][j] = PNPP_WS_MFMA(ra[buf][c][i].x, rb[buf][c][j].x, acc[i][j]);
                            acc[i][j] = PNPP_WS_MFMA(ra[buf][c][i].y, rb[buf][c][j].y, acc[i][j]);
                            acc[i][j] = PNPP_WS_MFMA(ra[buf][c][i].z, rb[buf][c][j].z, acc[i][j]);
                            acc[i][j] = PNPP_WS_MFMA(ra[buf][c][i].w, rb[buf][c][j].w, acc[i][j]);
                        }
            };
            bool looped = false;
            if constexpr (DENSE_A && EMODE == E_MASK_STATS) {
                if (inter) {
                    looped = true;
                    const size_t mn = (size_t)(tile + nworkers) * BM;
                    const float *pa = (AMODE == A_DZ_POOL ? A.z : A.a) + mn * A.lda;
                    const float *pz = A.z + mn * A.lda;
                    const float *pzp = E.zp + (size_t)m0 * E.ldc;
                    auto issue = [&](int u) {  // an eighth of the two load streams
                        constexpr int GP = (NG + 7) / 8, ZP = MT * NT * 2;
                        if (have_next) {
#pragma unroll
                            for (int g = 0; g < GP; ++g) {
                                const int i = u * GP + g;
                                if (i < NG) {
                                    rp[i] = *reinterpret_cast<const float4 *>(pa + (size_t)(i * RPP) * A.lda + offA);
                                    if constexpr (AMODE == A_DZ)
                                        rq[i] = *reinterpret_cast<const float4 *>(pz + (size_t)(i * RPP) * A.lda + offA);
                                }
                            }
                        }
#pragma unroll
                        for (int q = u * ZP; q < (u + 1) * ZP; ++q) {
                            const int r = q & 15, j = (q >> 4) % NT, i = (q >> 4) / NT;
                            const unsigned oz = (unsigned)(wm * TM + i * 32 + 4 * lh) * (unsigned)E.ldc + (unsigned)(n0 + wn * TN + j * 32 + l31);
                            zp[i][j][r] = pzp[(size_t)((r & 3) + 8 * (r >> 2)) * E.ldc + oz];
                        }
                    };
                    ld(0, 0);
#pragma unroll
                    for (int t = 0; t < 8; t += 2) {
                        ld(1, t + 1);
                        issue(t);
                        mm(0);
                        if (t + 2 < 8) ld(0, t + 2);
                        issue(t + 1);
                        mm(1);
                    }
                }
            }
            if (!looped) {
                ld(0, 0);
#pragma unroll 1
                for (int t = 0; t < 8; t += 2) {
                    ld(1, t + 1);
                    mm(0);
                    if (t + 2 < 8) ld(0, t + 2);
                    mm(1);
                }
            }
        } else {
            {
                // K loop, software-pipelined by hand: the LDS operand reads of block b+1 (SB k-steps) are issued before
                // the MFMAs of block b, so an MFMA never waits for a read issued right in front of it
                constexpr int SB = (KD / 2) % 4 == 0 ? 4 : 2, NBLK = (KD / 2) / SB;
                float ra[2][SB][MT], rb[2][SB][NT];
                auto ld = [&](int buf, int s0) {
    #pragma unroll
                    for (int u = 0; u < SB; ++u) {
    #pragma unroll
                        for (int i = 0; i < MT; ++i) ra[buf][u][i] = As[a_idx(wm * TM + i * 32 + l31, 2 * (s0 + u) + lh)];
    #pragma unroll
                        for (int j = 0; j < NT; ++j) rb[buf][u][j] = bp[2 * (s0 + u) * BN + j * 32];
                    }
                };
                auto mm = [&](int buf) {
    #pragma unroll
                    for (int u = 0; u < SB; ++u)
    #pragma unroll
                        for (int i = 0; i < MT; ++i)
    #pragma unroll
                            for (int j = 0; j < NT; ++j)
                                acc[i][j] = PNPP_WS_MFMA(ra[buf][u][i], rb[buf][u][j], acc[i][j]);
                };
                ld(0, 0);
    #pragma unroll 1
                for (int blk = 0; blk + 1 < NBLK; blk += 2) {  // rolled: a fully unrolled loop lets the scheduler hoist reads until it spills
                    ld(1, (blk + 1) * SB);
                    mm(0);
                    if (blk + 2 < NBLK) ld(0, (blk + 2) * SB);
                    mm(1);
                }
                if constexpr (NBLK % 2 == 1) mm(0);
            }
        }

        PNPP_STAMP(4)
        // epilogue: each accumulator register is one row; a half-wave writes 32 consecutive floats (128 B)
        bool done = false;
        if constexpr (EMODE != E_MASK_STATS) {
            // interior tiles of the forward kernels: no bounds tests, and every store is (uniform row pointer) + (one 32-bit
            // lane offset) -- scalar address arithmetic instead of a 64-bit multiply-add, a compare and an EXEC branch per row
            if (m0 + BM <= M && n0 + BN <= Nout) {
                done = true;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        float *tb = E.c + (size_t)(m0 + wm * TM + i * 32) * E.ldc + (n0 + wn * TN + j * 32);
                        const unsigned lo = (unsigned)(4 * lh) * (unsigned)E.ldc + (unsigned)l31;
                        float t1 = 0.f, t2 = 0.f;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float v = acc[i][j][r];
                            float *tr = tb + (size_t)((r & 3) + 8 * (r >> 2)) * E.ldc;
                            if constexpr (!DEFER) {
                                if (!PNPP_WS_EXP_NO_STORE) tr[lo] = v;
                            }
                            t1 += v;
                            t2 = fmaf(v, v, t2);
                        }
                        if constexpr (DEFER) held = acc[i][j], held_m0 = m0;
                        if constexpr (EMODE == E_STORE_STATS) s1[j] += (double)t1, s2[j] += (double)t2;
                        if constexpr (EMODE == E_STORE_STATS) {
                            if (E.pool_ext) {   // (uniform) this 32 x 32 tile is one neighbourhood: its extreme row per column
                                const float sg = pool_sg[j];
                                float mx = sg * acc[i][j][0];
#pragma unroll
                                for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sg * acc[i][j][r]);
                                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));        // the other 16 rows of the column sit in lane ^ 32
                                int a = 64;
#pragma unroll
                                for (int r = 15; r >= 0; --r) a = (sg * acc[i][j][r] == mx) ? (r & 3) + 8 * (r >> 2) + 4 * lh : a;
                                a = min(a, __shfl_xor(a, 32, 64));             // first row attaining it
                                if constexpr (DEFER) {   // stored with the tile, behind the next staging pass
                                    held_ext = sg * mx, held_arg = a;
                                } else if (lh == 0) {
                                    const size_t gi = (size_t)((m0 + wm * TM + i * 32) >> 5) * E.ldc + (n0 + wn * TN + j * 32 + l31);
                                    E.pool_ext[gi] = sg * mx;
                                    E.pool_arg[gi] = a;
                                }
                            }
                        }
                    }
            }
        }
        if constexpr (EMODE == E_MASK_STATS && NT == 1) {  // (two column tiles per wave: hipcc hoists the straight-line copy into spills)
            if (m0 + BM <= M && n0 + BN <= Nout) {  // the same for the backward kernels: ReLU mask, BN-backward sums, a_{l-1} tile
                done = true;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const int col = n0 + wn * TN + j * 32 + l31;
                        const float sc = E.scale[col], sh = E.shift[col], mu = E.mu[col], is = E.istd[col];
                        float *tb = E.c + (size_t)(m0 + wm * TM + i * 32) * E.ldc + (n0 + wn * TN + j * 32);
                        const unsigned lo = (unsigned)(4 * lh) * (unsigned)E.ldc + (unsigned)l31;
                        float *apb = Ap + (wm * TM + i * 32 + 4 * lh) * BN + wn * TN + j * 32 + l31;
                        float t1 = 0.f, t2 = 0.f;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float z0 = zp[i][j][r];
                            const float a0 = fmaf(z0, sc, sh);
                            const float v = a0 > 0.f ? acc[i][j][r] : 0.f;
                            float *tr = tb + (size_t)((r & 3) + 8 * (r >> 2)) * E.ldc;
                            if (!PNPP_WS_EXP_NO_STORE) tr[lo] = v;
                            t1 += v;
                            t2 = fmaf(v, (z0 - mu) * is, t2);
                            if constexpr (FDW) apb[((r & 3) + 8 * (r >> 2)) * BN] = fmaxf(a0, 0.f);
                        }
                        s1[j] += (double)t1, s2[j] += (double)t2;
                    }
            }
        }
        if (!done)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = n0 + wn * TN + j * 32 + l31;
                float sc = 0.f, sh = 0.f, mu = 0.f, is = 0.f;
                if constexpr (EMODE == E_MASK_STATS) {
                    const int cc = min(col, Nout - 1);
                    sc = E.scale[cc], sh = E.shift[cc], mu = E.mu[cc], is = E.istd[cc];
                }
                // statistics: this lane's 16 rows are summed in float32, the tiles of the worker in float64 (a float64
                // add per element costs several VALU slots, and VALU time is MFMA time here)
                float t1 = 0.f, t2 = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const bool ok = row < M && col < Nout;
                    float v = ok ? acc[i][j][r] : 0.f;
                    if constexpr (EMODE == E_STORE_STATS) {
                        t1 += v;
                        t2 = fmaf(v, v, t2);
                    } else if constexpr (EMODE == E_MASK_STATS) {
                        const float z0 = zp[i][j][r];
                        v = (fmaf(z0, sc, sh) > 0.f) ? v : 0.f;
                        t1 += v;
                        t2 = fmaf(v, (z0 - mu) * is, t2);
                    }
                    if (ok) E.c[(size_t)row * E.ldc + col] = v;
                    if constexpr (FDW) {  // a_{l-1} = relu(bn(z_{l-1})), the operand dW_l is contracted with
                        const int rl = wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        Ap[rl * BN + wn * TN + j * 32 + l31] = fmaxf(fmaf(zp[i][j][r], sc, sh), 0.f);
                    }
                }
                if constexpr (EMODE != E_STORE) s1[j] += (double)t1, s2[j] += (double)t2;
            }
        PNPP_STAMP(5)
        if constexpr (FDW) {
            __syncthreads();  // the whole relu(bn(zp)) tile is in LDS; the dZ tile still is
            PNPP_STAMP(6)
            // dW tile (ct, kt) += dZ^T (columns ct*32.. of the A tile) x activation tile (columns kt*32..).  A wave's DT tiles
            // (tile_id = wave + 4 t) share kt, so one activation operand feeds DT MFMAs on DT independent accumulators.
            // The reduction index is the tile row m = 32 c + 2 t2 + lh; f(m) = f(2 t2) | (lh << 2) (the swizzle only looks at
            // m mod 16), so the swizzled column is ((ct*32 + l31) ^ (lh << 2)) ^ F(t2) with F(t2) = (t2 & 7) << 3 uniform:
            // scalar work plus one xor per tile and t2, and the BM / 32 reads of a t2 differ by immediate offsets only.
            static_assert(4 % (BN / 32) == 0, "a wave's dW tiles must share their activation columns");
            constexpr int MC = BM / 32;
            const int kt = wave % (BN / 32);
            int colx[DT];
#pragma unroll
            for (int t = 0; t < DT; ++t) colx[t] = (((wave + 4 * t) / (BN / 32)) * 32 + l31) ^ (lh << 2);
            const float *abase = As + lh * KP, *bbase = Ap + lh * BN + kt * 32 + l31;
            float da[2][MC][DT], db[2][MC];
            auto ld = [&](int buf, int t2) {
                const int F = (t2 & 7) << 3;
                const float *pb = bbase + 2 * t2 * BN;
#pragma unroll
                for (int c = 0; c < MC; ++c) db[buf][c] = pb[32 * c * BN];
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const float *pa = abase + 2 * t2 * KP + (colx[t] ^ F);
#pragma unroll
                    for (int c = 0; c < MC; ++c) da[buf][c][t] = pa[32 * c * KP];
                }
            };
            auto mm = [&](int buf) {
#pragma unroll
                for (int c = 0; c < MC; ++c)
#pragma unroll
                    for (int t = 0; t < DT; ++t)
                        dwacc[t] = PNPP_WS_MFMA(da[buf][c][t], db[buf][c], dwacc[t]);
            };
            if constexpr (ONE_WAVE || TUNED_128) {
                // one wave per SIMD here, registers to spare: the swizzled operand addresses of the eight F values are a table
                // built once per tile from this lane's colx, and with t2 unrolled every read of the loop is (table entry) +
                // (immediate offset) -- no address arithmetic between the MFMAs (it was 45 VALU per 8 MFMAs)
                const float *pre[DT][8];
#pragma unroll
                for (int t = 0; t < DT; ++t)
#pragma unroll
                    for (int f = 0; f < 8; ++f) pre[t][f] = abase + 2 * f * KP + (colx[t] ^ (f << 3));
                auto ldt = [&](int buf, int t2) {
                    const int f = t2 & 7, h = t2 >> 3;
                    const float *pb = bbase + 2 * t2 * BN;
#pragma unroll
                    for (int c = 0; c < MC; ++c) db[buf][c] = pb[32 * c * BN];
#pragma unroll
                    for (int t = 0; t < DT; ++t) {
                        const float *pa = pre[t][f] + 16 * h * KP;
#pragma unroll
                        for (int c = 0; c < MC; ++c) da[buf][c][t] = pa[32 * c * KP];
                    }
                };
                ldt(0, 0);
#pragma unroll
                for (int t2 = 0; t2 < 16; t2 += 2) {
                    ldt(1, t2 + 1);
                    mm(0);
                    if (t2 + 2 < 16) ldt(0, t2 + 2);
                    mm(1);
                }
            } else {
                ld(0, 0);
#pragma unroll 1
                for (int t2 = 0; t2 < 16; t2 += 2) {
                    ld(1, t2 + 1);
                    mm(0);
                    if (t2 + 2 < 16) ld(0, t2 + 2);
                    mm(1);
                }
            }
            PNPP_STAMP(7)
        }
    }

    flush_held();
    PNPP_STAMP(9)       // (nothing: closes the last tile)
    if constexpr (FDW) {  // one partial dW per worker: dwslab[worker][c][n0 + k]
      if (n0 + BN <= Nout) {  // (uniform row pointer) + (one lane offset): scalar address arithmetic, no bounds test per element
        float *wb = E.dwslab + (size_t)worker * KD * E.dw_ld + n0;
        const unsigned lo = (unsigned)(4 * lh) * (unsigned)E.dw_ld + (unsigned)l31;
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            const int tile_id = wave + 4 * t, ct = tile_id / (BN / 32), kt = tile_id % (BN / 32);
            float *tb = wb + (size_t)(ct * 32) * E.dw_ld + kt * 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) tb[(size_t)((r & 3) + 8 * (r >> 2)) * E.dw_ld + lo] = dwacc[t][r];
        }
      } else
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            const int tile_id = wave + 4 * t, ct = tile_id / (BN / 32), kt = tile_id % (BN / 32);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, k = n0 + kt * 32 + l31;
                if (k < Nout) E.dwslab[((size_t)worker * KD + c) * E.dw_ld + k] = dwacc[t][r];
            }
        }
    }

    if constexpr (EMODE != E_STORE) {
        __syncthreads();
        double *red = reinterpret_cast<double *>(lds);  // [WM][2][BN]; the launcher sizes the LDS for it as well
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
        for (int f = tid; f < 2 * BN; f += 256) {
            const int which = f / BN, cl = f % BN;
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < WM; ++w) t += red[(w * 2 + which) * BN + cl];
            if (n0 + cl < Nout) E.slab[((size_t)worker * 2 + which) * Nout + n0 + cl] = t;
        }
    }
    PNPP_STAMP(10)      // tail: dW partial, statistics slab (stores complete)
}

template <int KD, int BM, int BN, int WM, int WN, int AM, int EM, bool FDW>
static int launch_ws_one(const AOperand &A, const BOperand &B, int M, int Nout, const Epilogue &E, int *nslab, hipStream_t st,
                         int *dw_slabs) {
    const int tiles = cdiv(M, BM), ncol = cdiv(Nout, BN);
    size_t lds = ((size_t)KD * BN + (size_t)BM * (KD % 32 == 0 ? KD : KD + 1) + (FDW ? (size_t)BM * BN : 0)) * sizeof(float);
    const size_t red_bytes = (size_t)WM * 2 * BN * sizeof(double);  // column-statistics reduction reuses the LDS
    if (lds < red_bytes) lds = red_bytes;
    // persistent workers: as many workgroups as the LDS lets the chip hold at once (dW slabs and statistic slabs are
    // per worker, so fewer is cheaper), at most three per CU
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 3) per_cu = 3;
    if (per_cu < 1) per_cu = 1;
    const int workers = worker_count((256 * per_cu) / ncol, tiles, 1);
    if (nslab) *nslab = workers;
    if (dw_slabs) *dw_slabs = FDW ? workers : 0;
    ProfScope ps(st, "gemm_ws_kernel<%d,%d,%d,A%d,E%d%s> M=%d N=%d K=%d grid=%dx1", KD, BM, BN, AM, EM, FDW ? ",dW" : "", M, Nout,
                 KD, workers * ncol);
    constexpr auto kfn = gemm_ws_kernel<KD, BM, BN, WM, WN, AM, EM, FDW>;
    grant_lds<kfn>(lds);
    hipLaunchKernelGGL(kfn, dim3(workers * ncol), dim3(256), lds, st, A, B, M, Nout, ncol, E);
    PNPP_CHECK_LAUNCH("gemm_ws");
    return PNPP_OK;
}

template <int KD, int BM, int BN, int WM, int WN, int AM>
static int launch_ws_e(const AOperand &A, const BOperand &B, int M, int Nout, const Epilogue &E, int *nslab, hipStream_t st,
                       int *dw_slabs = nullptr) {
    if (dw_slabs) *dw_slabs = 0;
    switch (E.mode) {
        case E_STORE: return launch_ws_one<KD, BM, BN, WM, WN, AM, E_STORE, false>(A, B, M, Nout, E, nslab, st, nullptr);
        case E_STORE_STATS: return launch_ws_one<KD, BM, BN, WM, WN, AM, E_STORE_STATS, false>(A, B, M, Nout, E, nslab, st, nullptr);
        case E_MASK_STATS:
            if constexpr ((AM == A_DZ || AM == A_DZ_POOL) && KD % 32 == 0 && ((KD / 32) * (BN / 32)) % 4 == 0) {
                if (E.dwslab && dw_slabs)
                    return launch_ws_one<KD, BM, BN, WM, WN, AM, E_MASK_STATS, true>(A, B, M, Nout, E, nslab, st, dw_slabs);
            }
            return launch_ws_one<KD, BM, BN, WM, WN, AM, E_MASK_STATS, false>(A, B, M, Nout, E, nslab, st, nullptr);
    }
    set_error("gemm_ws: bad epilogue mode %d", E.mode);
    return PNPP_ERR_ARG;
}

// dense (non-grouped) operands: K in {64, 128, 256}
template <int KD, int BM, int BN, int WM, int WN>
static int launch_ws_dense(const AOperand &A, const BOperand &B, int M, int Nout, const Epilogue &E, int *nslab, hipStream_t st,
                           int *dw_slabs) {
    switch (A.mode) {
        case A_PLAIN: return launch_ws_e<KD, BM, BN, WM, WN, A_PLAIN>(A, B, M, Nout, E, nslab, st);
        case A_BNRELU: return launch_ws_e<KD, BM, BN, WM, WN, A_BNRELU>(A, B, M, Nout, E, nslab, st);
        case A_DZ: return launch_ws_e<KD, BM, BN, WM, WN, A_DZ>(A, B, M, Nout, E, nslab, st, dw_slabs);
        case A_DZ_POOL: return launch_ws_e<KD, BM, BN, WM, WN, A_DZ_POOL>(A, B, M, Nout, E, nslab, st, dw_slabs);
    }
    set_error("gemm_ws: bad A mode %d", A.mode);
    return PNPP_ERR_ARG;
}

// picks a weights-stationary configuration, or returns false when the shape does not qualify (the chunked kernel
// then handles it): the reference models' grouped layers all qualify
bool try_launch_ws(const AOperand &A, const BOperand &B, int M, int Nout, int Kd, const Epilogue &E, int *nslab, hipStream_t st, int *rc,
                   int *dw_slabs) {
    if (M < 8192 || Nout % 64 != 0) return false;
    const bool grouped = A.mode == A_GATHER || A.mode == A_CONCAT;
    if (grouped) {
        if (Kd != A.D + 4) return false;
        if (A.mode != A_GATHER) return false;
        if (A.D == 0) {  // xyz only
            if (Nout % 128 == 0) *rc = launch_ws_e<4, 128, 128, 4, 1, A_GATHER>(A, B, M, Nout, E, nslab, st);
            else *rc = launch_ws_e<4, 128, 64, 4, 1, A_GATHER>(A, B, M, Nout, E, nslab, st);
            return true;
        }
        if (A.D == 128 && ((uintptr_t)A.a & 15) == 0) {
            *rc = launch_ws_e<132, 64, 64, 2, 2, A_GATHER>(A, B, M, Nout, E, nslab, st);
            return true;
        }
        return false;
    }
    if (A.lda % 4 != 0 || ((uintptr_t)A.a & 15) != 0) return false;
    if (Kd == 64) {   // 64 x 64 tiles for every K = 64 launch (measured against 128 x 128 / 128 x 64: forward 30.0 vs 31.9 and 19.3 vs
                      // 19.4 us, backward 36.7 vs 40.5 us on SA1: twice the tiles per worker, column blocks share an XCD's L2)
        *rc = launch_ws_dense<64, 64, 64, 2, 2>(A, B, M, Nout, E, nslab, st, dw_slabs);
        return true;
    }
    if (Kd == 128) {
        // (a 128-row tile with one workgroup per CU and the K = 256 kernel's unrolled, interleaved loops was measured at the same
        // 57.8 us for the SA1 backward launch and 4-7 % slower for the others)
        *rc = launch_ws_dense<128, 64, 64, 2, 2>(A, B, M, Nout, E, nslab, st, dw_slabs);
        return true;
    }
    if (Kd == 256) {
        *rc = launch_ws_dense<256, 64, 64, 2, 2>(A, B, M, Nout, E, nslab, st, dw_slabs);
        return true;
    }
    return false;
}

unsigned gemm_build_flags() { return ((PNPP_WS_EXP_NO_MFMA != 0) ? 1u : 0u) | stamps_bit(); }

}  // namespace pnpp

#ifdef PNPP_STAMPS
extern "C" int pnpp_debug_stamps(unsigned long long *out16, int kd) {  // kd > 0: select + reset; kd == 0: read
    if (kd > 0) {
        unsigned long long z[16] = {0};
        hipMemcpyToSymbol(HIP_SYMBOL(pnpp::g_stamps), z, sizeof(z));
        hipMemcpyToSymbol(HIP_SYMBOL(pnpp::g_stamp_kd), &kd, sizeof(int));
    } else {
        hipDeviceSynchronize();
        hipMemcpyFromSymbol(out16, HIP_SYMBOL(pnpp::g_stamps), 16 * sizeof(unsigned long long));
    }
    return 0;
}
#endif
