// gemm_wsf3_kernels.hip -- the forward 1x1 convolutions of the grouped levels (gemm_wsf_kernels.hip: wave-private 32-row strips, no
// barrier in the strip loop) with the float32 products formed on the bf16 matrix pipe from EXACT three-way operand splits.
//
// Reference: models/pointnet_pp_8dir.py:40-42 (conv -> BatchNorm -> ReLU), float32.
//
// The arithmetic of the split (why three pieces, which six products, why two accumulators): split_prims.h.
//
// Layout.  Per wave 3 planes [32 rows][64 k] bf16 of its strip chunk (128-byte rows, 16-byte groups XOR-swizzled by x(r) = 4 bit1(r) +
// bits3:2(r): the four 16-lane groups of a ds_read_b128 then touch all 64 banks once); per workgroup 3 planes [64 n][KD] bf16 of the weight panel.
// K = 64: 4 waves, 24 + 48 = 72 KB, two workgroups per CU; K = 128: 8 waves, 48 + 96 = 144 KB, one workgroup per CU -- eight waves per
// CU either way: while one wave of a SIMD splits and stages (VALU), the other multiplies (an MFMA holds the vector issue for 8 of its
// 32 cycles only).
#include "launch.h"
#include "split_prims.h"

namespace pnpp {

// KD in {64, 128}; NW waves per workgroup; NT column tiles of 32 per wave; AX = A_PLAIN or A_BNRELU; EM = E_STORE or E_STORE_STATS
template <int KD, int NW, int NT, int AX, int EM>
__global__ void __launch_bounds__(NW * 64, NW == 4 ? 2 : 1)
gemm_wsf3_kernel(const float *__restrict__ A, int lda, const float *__restrict__ scale, const float *__restrict__ shift,
                 const float *__restrict__ W, int ldw, int M, int Nout, int ncol, const Epilogue E) {
    constexpr int BN = NT * 32, NC = KD / 64, NTHR = NW * 64;
    constexpr int WPITCH = KD * 2, WPLANE = BN * WPITCH;   // bytes: a row and a plane of the weight panel
    constexpr int APLANE = 32 * 128, ASTRIP = 3 * APLANE;  // bytes: a plane of a strip chunk, a wave's three planes
    constexpr int WCH = KD / 8;                            // 16-byte groups per panel row
    extern __shared__ __attribute__((aligned(16))) unsigned char lds3[];
    unsigned char *Wp = lds3;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned char *Ap = lds3 + 3 * WPLANE + wave * ASTRIP;
    const int l31 = lane & 31, lh = lane >> 5;
    auto swzW = [](int n) { return WCH >= 16 ? (n & 15) : ((n >> 1) & 7); };

    // XCD-aware map (as gemm_wsf_kernel): the column blocks of one worker sit on one XCD and share its L2
    const int nworkers = gridDim.x / ncol;
    int col_blk = blockIdx.x % ncol, worker = blockIdx.x / ncol;
    if ((nworkers & 7) == 0) {
        const int xcd = blockIdx.x & 7, i = blockIdx.x >> 3;
        col_blk = i % ncol, worker = (i / ncol) * 8 + xcd;
    }
    const int n0 = col_blk * BN;
    const bool wt_stream = (E.store_policy & ST_STREAMS) != 0, wt_stats = (E.store_policy & ST_STAT_SLABS) != 0;

    // per-channel constants of this lane's column group (k = 64 c + 4 q .. + 3)
    const int q = lane & 15, q4 = 4 * q, rb = lane >> 4;   // staging map: column group lane % 16, rows lane / 16 + 4 i
    float4 sc[NC], sh[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        sc[c] = make_float4(1.f, 1.f, 1.f, 1.f), sh[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (AX == A_BNRELU) {
            sc[c] = *reinterpret_cast<const float4 *>(scale + 64 * c + q4);
            sh[c] = *reinterpret_cast<const float4 *>(shift + 64 * c + q4);
        }
    }
    // weight panel W[n0 .. n0 + 64)[0 .. KD): consecutive lanes take consecutive 16-byte groups of one row; split once per workgroup
    {
        constexpr int NWF = (KD / 4) * BN / NTHR;
        f32x4 tw[NWF];
#pragma unroll
        for (int j = 0; j < NWF; ++j) {
            const int f = tid + NTHR * j, nl = f / (KD / 4), k4 = 4 * (f % (KD / 4));
            tw[j] = *reinterpret_cast<const f32x4 *>(W + (size_t)(n0 + nl) * ldw + k4);
        }
#pragma unroll
        for (int j = 0; j < NWF; ++j) {
            const int f = tid + NTHR * j, nl = f / (KD / 4), k4 = 4 * (f % (KD / 4));
            uint2 h, m, l;
            sp_split4(tw[j], h, m, l);
            unsigned char *dst = Wp + nl * WPITCH + 16 * ((k4 >> 3) ^ swzW(nl)) + 2 * (k4 & 7);
            *reinterpret_cast<uint2 *>(dst) = h;
            *reinterpret_cast<uint2 *>(dst + WPLANE) = m;
            *reinterpret_cast<uint2 *>(dst + 2 * WPLANE) = l;
        }
    }

    // strips: this wave takes strip (worker * NW + wave) + i * (nworkers * NW)
    const int nstrips = M / 32, stride = nworkers * NW;
    int strip = worker * NW + wave;
    const __amdgpu_buffer_rsrc_t resA = sp_buf_rsrc(A);
    const unsigned oa0 = 4u * ((unsigned)rb * (unsigned)lda + (unsigned)q4);   // rows rb + 4 i: the i part rides in the scalar offset
    f32x4 ra[NC][8];
    auto fetch = [&](int s) {
        const unsigned so = (unsigned)s * 32u * (unsigned)lda * 4u;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < 8; ++i) ra[c][i] = sp_buf_load4(resA, oa0, so + 256u * (unsigned)c + (unsigned)i * (16u * (unsigned)lda));
    };
    if (strip < nstrips) fetch(strip);

    double s1[NT], s2[NT];
    float sg[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        s1[j] = s2[j] = 0.0;
        sg[j] = 1.f;
        if constexpr (EM == E_STORE_STATS) {
            if (E.pool_ext && E.pool_gamma) sg[j] = E.pool_gamma[n0 + j * 32 + l31] >= 0.f ? 1.f : -1.f;
        }
    }
    __syncthreads();   // the weight panel is complete; from here on the waves run on their own

    // this lane's staging slot in a strip plane: row rb + 4 i, 8 bytes at k = q4 (half q & 1 of group q >> 1).  sp_swz_row(rb + 4 i) =
    // 4 bit1(rb) | (i & 3) as rb < 4: the i part is applied per store (^ ((i & 3) << 4), + 512 i), the rb part is spelled out here
    const unsigned wofs0 = (unsigned)(rb * 128 + 16 * ((q >> 1) ^ (((rb >> 1) & 1) << 2)) + 8 * (q & 1));
    const unsigned char *arow = Ap + l31 * 128;
    const int ax = sp_swz_row(l31);
    const unsigned char *brow[NT];
    int bx[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = j * 32 + l31;
        brow[j] = Wp + n * WPITCH;
        bx[j] = swzW(n);
    }
    // A strip's column tiles are multiplied two at a time (NH passes over the strip image: 64 accumulator registers per pass; the image is
    // staged, i.e. read, transformed and split, ONCE for all NT tiles)
    constexpr int NH = NT / 2;
    static_assert(NT == 2 || (NT == 4 && NC == 1), "four tiles per wave: one chunk (the passes re-read the chunk image)");
    // stage chunk c of the strip: transform and split in registers, three ds_write_b64 per group (in-order per wave: the reads of the
    // previous chunk were issued before these writes, and the reads that follow come after them)
    auto stage = [&](int c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f32x4 v = ra[c][i];
            if constexpr (AX == A_BNRELU) {
                v[0] = fmaxf(fmaf(v[0], sc[c].x, sh[c].x), 0.f), v[1] = fmaxf(fmaf(v[1], sc[c].y, sh[c].y), 0.f);
                v[2] = fmaxf(fmaf(v[2], sc[c].z, sh[c].z), 0.f), v[3] = fmaxf(fmaf(v[3], sc[c].w, sh[c].w), 0.f);
            }
            uint2 h, m, l;
            sp_split4(v, h, m, l);
            unsigned char *dst = Ap + (wofs0 ^ (unsigned)((i & 3) << 4)) + i * 512;
            *reinterpret_cast<uint2 *>(dst) = h;
            *reinterpret_cast<uint2 *>(dst + APLANE) = m;
            *reinterpret_cast<uint2 *>(dst + 2 * APLANE) = l;
        }
    };
    // tiles 2 hh, 2 hh + 1 of chunk c: step t covers k = 64 c + 16 t + 8 lh + (0 .. 7): group 2 t + lh of the strip chunk, group
    // 8 c + 2 t + lh of the panel rows
    auto product = [&](int c, int hh, f32x16 (&acc)[2], f32x16 (&accl)[2]) {
        uint4 fa[2][3], fb[2][2][3];
        auto ld = [&](int buf, int t) {
            const int g = 2 * t + lh;
#pragma unroll
            for (int p = 0; p < 3; ++p) fa[buf][p] = *reinterpret_cast<const uint4 *>(arow + p * APLANE + 16 * (g ^ ax));
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    fb[buf][j][p] = *reinterpret_cast<const uint4 *>(brow[2 * hh + j] + p * WPLANE + 16 * ((8 * c + g) ^ bx[2 * hh + j]));
        };
        auto mm = [&](int buf) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bf16x8 ah = sp_op(fa[buf][0]), am = sp_op(fa[buf][1]), al = sp_op(fa[buf][2]);
                const bf16x8 bh = sp_op(fb[buf][j][0]), bm = sp_op(fb[buf][j][1]), bl = sp_op(fb[buf][j][2]);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[j], 0, 0, 0);
                accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, accl[j], 0, 0, 0);
                accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, accl[j], 0, 0, 0);
                accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, accl[j], 0, 0, 0);
                accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, accl[j], 0, 0, 0);
                accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, accl[j], 0, 0, 0);
            }
        };
        ld(0, 0);
#pragma unroll
        for (int t = 0; t < 4; t += 2) {
            ld(1, t + 1);
            mm(0);
            if (t + 2 < 4) ld(0, t + 2);
            mm(1);
        }
    };
    // epilogue of tiles 2 hh, 2 hh + 1 of the strip: 16 rows of one column per lane and column tile
    auto epilogue = [&](int hh, f32x16 (&acc)[2], f32x16 (&accl)[2]) {
        float *tb = E.c + (size_t)(strip * 32 + 4 * lh) * E.ldc + n0 + l31;
        float t1[2] = {0.f, 0.f}, t2[2] = {0.f, 0.f};
        sp_with_policy(wt_stream, [&](auto wt) {   // ONE branch for both tiles' stores (a branch per tile cost the K = 64 launch 1.5 us of 27)
#pragma unroll
            for (int j2 = 0; j2 < 2; ++j2) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[j2][r] + accl[j2][r];
                    acc[j2][r] = v;
                    sp_store(tb + (size_t)((r & 3) + 8 * (r >> 2)) * E.ldc + (2 * hh + j2) * 32, v, wt());
                    t1[j2] += v, t2[j2] = fmaf(v, v, t2[j2]);
                }
            }
        });
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2) {
            const int j = 2 * hh + j2;
            if constexpr (EM == E_STORE_STATS) {
                s1[j] += (double)t1[j2], s2[j] += (double)t2[j2];
                if (E.pool_ext) {   // the strip is one neighbourhood: extreme pre-BN value per column and its first row
                    float mx = sg[j] * acc[j2][0];
#pragma unroll
                    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sg[j] * acc[j2][r]);
                    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                    int a = 64;
#pragma unroll
                    for (int r = 15; r >= 0; --r) a = (sg[j] * acc[j2][r] == mx) ? (r & 3) + 8 * (r >> 2) + 4 * lh : a;
                    a = min(a, __shfl_xor(a, 32, 64));
                    if (lh == 0) {
                        const size_t gi = (size_t)strip * E.ldc + n0 + j * 32 + l31;
                        E.pool_ext[gi] = sg[j] * mx;
                        E.pool_arg[gi] = a;
                    }
                }
            }
        }
    };
    for (; strip < nstrips; strip += stride) {
        if constexpr (NH == 1) {
            f32x16 acc[2], accl[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f, accl[j][r] = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                stage(c);
                if (c == NC - 1 && strip + stride < nstrips) fetch(strip + stride);   // the next strip flies during the MFMAs
                product(c, 0, acc, accl);
            }
            epilogue(0, acc, accl);
        } else {
            stage(0);
            if (strip + stride < nstrips) fetch(strip + stride);
#pragma unroll
            for (int hh = 0; hh < NH; ++hh) {
                f32x16 acc[2], accl[2];
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f, accl[j][r] = 0.f;
                product(0, hh, acc, accl);
                epilogue(hh, acc, accl);
                __builtin_amdgcn_sched_barrier(0);   // (the scheduler would overlap the passes: their accumulators do not fit together)
            }
        }
    }

    if constexpr (EM == E_STORE_STATS) {
        // per-column sums of this worker: lane halves, then the waves in wave order
        __syncthreads();   // every wave is done with the panel and its strip
        double *red = reinterpret_cast<double *>(lds3);   // [NW waves][2][BN]
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const double a = s1[j] + shfl_xor_f64(s1[j], 32), b = s2[j] + shfl_xor_f64(s2[j], 32);
            if (lh == 0) red[(wave * 2 + 0) * BN + j * 32 + l31] = a, red[(wave * 2 + 1) * BN + j * 32 + l31] = b;
        }
        __syncthreads();
        for (int f = tid; f < 2 * BN; f += NTHR) {
            const int which = f / BN, cl = f % BN;
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += red[(w * 2 + which) * BN + cl];
            sp_store(E.slab + ((size_t)worker * 2 + which) * Nout + n0 + cl, t, wt_stats);
        }
    }
}

// 1 (default): the float32 products of the grouped layers' large GEMMs on v_mfma_f32_32x32x16_bf16 from exact three-way operand splits
// (this file, gemm_wsd3_kernels.hip); 0: on v_mfma_f32_32x32x2_f32 (PNPP_SPLIT_PRODUCTS=0 / pnpp_set_split_products)
static int g_split_products = -1;
int split_products() {
    if (g_split_products < 0) g_split_products = env_int("PNPP_SPLIT_PRODUCTS", 1) != 0;
    return g_split_products;
}
void set_split_products(int on) { g_split_products = on ? 1 : 0; }

// Which classes of store sites write through (common.h: StorePolicy).  No environment switch: pnpp_set_store_policy is the one way in.
// Ships: the dW partial slabs and the streamed outputs; the float64 statistics slabs stay plain (no launch moved with them).  What each
// class measured: profiles/store_policy_kernel_stats.csv, DESIGN.md section 9.
static int g_store_policy = ST_DW_SLABS | ST_STREAMS;
int store_policy() { return g_store_policy; }
void set_store_policy(int mask) { g_store_policy = mask & ST_ALL; }

template <int KD, int NW, int NT, int AX, int EM>
static void wsf3_launch(const AOperand &A, const BOperand &B, int M, int Nout, const Epilogue &E, int workers, int ncol, hipStream_t st) {
    constexpr size_t lds = (size_t)3 * (NT * 32) * KD * 2 + (size_t)NW * 3 * 32 * 128;
    static_assert(lds <= 160 * 1024, "LDS budget");
    constexpr auto kfn = gemm_wsf3_kernel<KD, NW, NT, AX, EM>;
    grant_lds<kfn>(lds);
    hipLaunchKernelGGL(kfn, dim3(workers * ncol), dim3(NW * 64), lds, st, A.a, A.lda, A.scale, A.shift, B.b, B.ldb, M, Nout, ncol, E);
}

// the shapes gemm_wsf_kernel takes (wsf_applies), when split products are on
bool try_launch_wsf3(const AOperand &A, const BOperand &B, int M, int Nout, int Kd, const Epilogue &E, int *nslab, hipStream_t st, int *rc) {
    *rc = PNPP_OK;
    if (!split_products() || !wsf_applies(A, B, M, Nout, Kd, E)) return false;
    // two column tiles per wave.  (PNPP_WSF3_NT4=1: four tiles per wave for K = 64 with 128 or more columns -- the strip is read, transformed
    // and split once for 128 columns, eight waves in one workgroup per CU -- measured 23.2 - 23.6 us against 22.6 us on the sa1 launch: the
    // launch is bound by its 67 MB of stores and by latency, not by the vector work the form saves)
    static const bool nt4_on = env_int("PNPP_WSF3_NT4", 0) != 0;
    const bool nt4 = nt4_on && Kd == 64 && Nout % 128 == 0;
    const int BNsel = nt4 ? 128 : 64, ncol = Nout / BNsel, nstrips = M / 32;
    const int NW = (Kd == 64 && !nt4) ? 4 : 8;
    const int workers = worker_count((NW == 4 ? 512 : 256) / ncol, nstrips, NW);   // eight waves per CU either way
    if (nslab) *nslab = workers;
    ProfScope ps(st, "gemm_wsf3_kernel<%d,A%d,E%d> M=%d N=%d K=%d grid=%dx1", Kd, A.mode, E.mode, M, Nout, Kd, workers * ncol);
    if (Kd == 64 && nt4) dispatch_ae(A.mode, E.mode, [&](auto am, auto em) { wsf3_launch<64, 8, 4, am(), em()>(A, B, M, Nout, E, workers, ncol, st); });
    else if (Kd == 64) dispatch_ae(A.mode, E.mode, [&](auto am, auto em) { wsf3_launch<64, 4, 2, am(), em()>(A, B, M, Nout, E, workers, ncol, st); });
    else dispatch_ae(A.mode, E.mode, [&](auto am, auto em) { wsf3_launch<128, 8, 2, am(), em()>(A, B, M, Nout, E, workers, ncol, st); });
    check_launch("gemm_wsf3", rc);
    return true;
}

}  // namespace pnpp

extern "C" int pnpp_set_split_products(int on) {
    pnpp::set_split_products(on);
    return PNPP_OK;
}
extern "C" int pnpp_get_split_products(void) { return pnpp::split_products(); }
extern "C" int pnpp_set_store_policy(int mask) {
    if (mask < 0 || mask > pnpp::ST_ALL) {
        pnpp::set_error("pnpp_set_store_policy: mask %d has bits outside %d", mask, (int)pnpp::ST_ALL);
        return PNPP_ERR_ARG;
    }
    pnpp::set_store_policy(mask);
    return PNPP_OK;
}
extern "C" int pnpp_get_store_policy(void) { return pnpp::store_policy(); }
