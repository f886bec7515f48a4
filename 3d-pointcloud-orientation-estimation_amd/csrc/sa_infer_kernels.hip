// sa_infer_kernels.hip -- forward-only (inference) path of PointNetSetAbstraction: one launch per level.
//
// Reference: models/pointnet_pp_8dir.py:21-43 evaluated with BatchNorm in eval mode.  With running statistics a BatchNorm is an
// affine map and folds into the 1x1 convolution in front of it (bn_fold_kernel, float64, rounded once):
//     a = gamma / sqrt(running_var + eps),   W' = a (.) W (row-wise),   b' = (b - running_mean) * a + beta
// so a level is  gather -> 3 x (GEMM + bias + ReLU) -> max over the neighbourhood.
//
// sa_infer_kernel: a workgroup (4 waves) owns TM rows = TM / K whole neighbourhoods.
//   1. builds the layer-0 operand [xyz[nbr] - xyz[centre] | points[nbr] | 0] (group_all: absolute coordinates) in LDS,
//   2. runs the three products as float32 products on the bf16 matrix pipe from EXACT three-way operand splits (the form of
//      csrc/gemm_wsf3_kernels.hip: six v_mfma_f32_32x32x16_bf16 per 16 reduction steps, float32 accumulation, 2.67 x the rate of
//      v_mfma_f32_32x32x2_f32, same parity gates).  The weights are constant between calls, so their three planes are written ONCE at
//      fold time, in the order the lanes read them (one 16-byte load per lane and plane per step, 1 KiB contiguous per wave,
//      L2-resident); an activation is split once, by the lane that produces it, as it is stored into the LDS planes the next
//      layer reads as its A operand -- nothing is re-split,
//   3. hands layer l's output tile (accumulators + b', ReLU, three bf16 planes) to layer l+1 through LDS,
//   4. takes the max over the K rows of each group from layer 2's accumulators and writes (B, S, C_2) only.
// No M x C tensor is written to global memory.  When the level has fewer row tiles than the chip has CUs (group_all levels), the
// columns of the LAST layer are split over blockIdx.y and every such workgroup recomputes layers 0 and 1 of its tile.
//
//
// sa_infer_wide_kernel: neighbourhoods larger than a row tile, K = 32 m rows (m = 2 .. 8).  A workgroup owns ONE neighbourhood and walks
// it in 32-row tiles: per tile it builds the layer-0 operand and runs the same three products; the column maxima of layer 2's
// accumulators are folded into a running maximum that stays in registers (a lane keeps one column of each of its wave's <= 8 column
// blocks), and (B, S, C_2) is written once, after the last tile.  Same LDS tiles, same weight blob, same column split of the last
// layer over blockIdx.y when there are fewer neighbourhoods than CUs (group_all levels over 64 .. 256 rows).
//
// Shapes taken (pnpp_sa_infer_supported): L == 3; C[l] multiples of 32, <= 1024; K = 16 or a multiple of 32 up to 256 (group_all: N
// likewise); D + 3 <= 1024; the two LDS tiles (three bf16 planes each) of a 32-row workgroup fit 160 KiB.
#include "kernels.h"
#include "split_infer.h"

namespace pnpp {

// workgroups a launch should reach before the last layer's columns stop being split: one per CU of the current device.
// Cached process-wide, unsynchronised, like the library's other process state (one process drives one GPU: pnpp_hip.dist)
int infer_target_wgs() {
    static int cus = 0;
    if (cus <= 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            return 256;   // no device (descriptor queries on a CPU-only machine): an MI355X's count; not cached
        cus = n;
    }
    return cus;
}

namespace {

constexpr int kInferThreads = 256;
constexpr int kInferMaxLds = 160 * 1024;
constexpr int kInferMaxK = 256;   // rows of a neighbourhood the wide kernel walks (8 tiles)

struct InferPlan {
    int TM;        // rows per workgroup (32 or 64)
    bool wide;     // K > 32: one neighbourhood per workgroup, walked in 32-row tiles (sa_infer_wide_kernel)
    int Kd0;       // layer 0's reduction length, padded to a multiple of 16
    int ldA, ldB;  // row strides of the two LDS tiles (bf16 elements)
    int nsplit;    // column split of the last layer over blockIdx.y
    int ntiles;
    size_t lds;
};

struct InferBlob {
    unsigned short *w[3];
    float *b[3];
    size_t woff[3], boff[3];   // byte offsets of W'_l (three bf16 planes of C_l x ld_l, fragment-major) and b'_l (C_l), 256-byte aligned
    int ld[3];
    size_t bytes;
};

static int infer_plan(const pnpp_sa_desc *d, InferPlan *p) {
    PNPP_REQUIRE(d, PNPP_ERR_ARG, "sa_infer: null descriptor");
    PNPP_REQUIRE(d->B > 0 && d->N > 0 && d->S > 0 && d->K > 0 && d->D >= 0, PNPP_ERR_ARG, "sa_infer: bad geometry B=%d N=%d S=%d K=%d D=%d",
                 d->B, d->N, d->S, d->K, d->D);
    if (d->group_all) PNPP_REQUIRE(d->S == 1 && d->K == d->N, PNPP_ERR_ARG, "sa_infer: group_all needs S == 1 and K == N");
    PNPP_REQUIRE(d->L == 3, PNPP_ERR_ARG, "sa_infer: the fused kernel takes 3 layers, not %d", d->L);
    PNPP_REQUIRE(d->K == 16 || (d->K % 32 == 0 && d->K <= kInferMaxK), PNPP_ERR_ARG,
                 "sa_infer: the fused kernel takes neighbourhoods of K = 16 or a multiple of 32 up to %d rows, not K=%d", kInferMaxK, d->K);
    for (int l = 0; l < 3; ++l)
        PNPP_REQUIRE(d->C[l] > 0 && d->C[l] % 32 == 0 && d->C[l] <= 1024, PNPP_ERR_ARG,
                     "sa_infer: mlp channel %d (=%d) must be a multiple of 32 up to 1024", l, d->C[l]);
    PNPP_REQUIRE(d->D + 3 <= 1024, PNPP_ERR_ARG, "sa_infer: D=%d input channels exceed 1021", d->D);
    PNPP_REQUIRE((long long)d->B * d->S * d->K < (1ll << 31) && (long long)d->B * d->N * (d->D > 3 ? d->D : 3) < (1ll << 31), PNPP_ERR_ARG,
                 "sa_infer: B*S*K or B*N*D overflows int32");
    p->Kd0 = (d->D + 3 + 15) & ~15;
    const int wideA = p->Kd0 > d->C[1] ? p->Kd0 : d->C[1];
    p->ldA = wideA + 8;   // bf16 elements; + 16 bytes: the 32 rows of a 16-byte-per-lane read fall on different banks
    p->ldB = d->C[0] + 8;
    const size_t per_row = (size_t)(p->ldA + p->ldB) * 3 * sizeof(unsigned short);   // three bf16 planes per tile
    const long long M = (long long)d->B * d->S * d->K;
    p->wide = d->K > 32;
    if (64 * per_row <= 80 * 1024 && M > 32 && !p->wide)
        p->TM = 64;   // two workgroups per CU still fit
    else
        p->TM = 32;
    p->lds = p->TM * per_row;
    PNPP_REQUIRE(p->lds <= (size_t)kInferMaxLds, PNPP_ERR_ARG, "sa_infer: a 32-row tile of widths %d and %d needs %zu bytes of LDS (> %d)", wideA,
                 d->C[0], p->lds, kInferMaxLds);
    p->ntiles = p->wide ? d->B * d->S : (int)((M + p->TM - 1) / p->TM);   // workgroups along x
    int ns = 1;
    const int ncb = d->C[2] / 32;
    const int target = infer_target_wgs();
    while (p->ntiles * ns < target && ncb % (ns * 2) == 0 && d->C[2] / (ns * 2) >= 128) ns *= 2;
    p->nsplit = ns;
    return PNPP_OK;
}

static InferBlob infer_blob(const pnpp_sa_desc *d, const InferPlan &p, void *base) {
    InferBlob b;
    size_t off = 0;
    char *cb = static_cast<char *>(base);
    for (int l = 0; l < 3; ++l) {
        b.ld[l] = l == 0 ? p.Kd0 : d->C[l - 1];
        b.woff[l] = off;
        off = align_up(off + (size_t)d->C[l] * b.ld[l] * 3 * sizeof(unsigned short), 256);
        b.boff[l] = off;
        off = align_up(off + (size_t)d->C[l] * sizeof(float), 256);
        b.w[l] = cb ? reinterpret_cast<unsigned short *>(cb + b.woff[l]) : nullptr;
        b.b[l] = cb ? reinterpret_cast<float *>(cb + b.boff[l]) : nullptr;
    }
    b.bytes = off;
    return b;
}

// W' (C x ld row-major, zero beyond Cin) and b' (C) of one linear + eval-mode BatchNorm pair (head blocks); float64, one rounding
__global__ __launch_bounds__(256) void bn_fold_kernel(const float *__restrict__ w, int Cin, const float *__restrict__ b,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      const float *__restrict__ rm, const float *__restrict__ rv, float eps, int ld,
                                                      float *__restrict__ wout, float *__restrict__ bout) {
    const int n = blockIdx.x;
    const double a = (double)gamma[n] / sqrt((double)rv[n] + (double)eps);
    for (int k = threadIdx.x; k < ld; k += blockDim.x)
        wout[(size_t)n * ld + k] = k < Cin ? (float)(a * (double)w[(size_t)n * Cin + k]) : 0.f;
    if (threadIdx.x == 0) bout[n] = (float)(((double)b[n] - (double)rm[n]) * a + (double)beta[n]);
}

// The same fold for a level's layer, W' written ONCE as the three bf16 planes sa_infer_kernel multiplies with, each in the order its
// lanes read ("fragment-major"): plane p, element (n, k) at p * C * ld + (((n/32) * (ld/16) + k/16) * 64 + 32 ((k%16)/8) + n%32) * 8 + k%8
__global__ __launch_bounds__(256) void bn_fold_split_kernel(const float *__restrict__ w, int Cin, const float *__restrict__ b,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            const float *__restrict__ rm, const float *__restrict__ rv, float eps, int ld,
                                                            unsigned short *__restrict__ wout, float *__restrict__ bout) {
    const int n = blockIdx.x;
    const size_t plane = (size_t)gridDim.x * ld;
    const double a = (double)gamma[n] / sqrt((double)rv[n] + (double)eps);
    for (int k = threadIdx.x; k < ld; k += blockDim.x) {
        const float v = k < Cin ? (float)(a * (double)w[(size_t)n * Cin + k]) : 0.f;
        unsigned h, m, l;
        sp_split2(v, 0.f, h, m, l);
        const size_t at = ((((size_t)(n >> 5) * (ld >> 4) + (k >> 4)) * 64 + (((k & 15) >> 3) << 5) + (n & 31)) << 3) + (k & 7);
        wout[at] = (unsigned short)h, wout[plane + at] = (unsigned short)m, wout[2 * plane + at] = (unsigned short)l;
    }
    if (threadIdx.x == 0) bout[n] = (float)(((double)b[n] - (double)rm[n]) * a + (double)beta[n]);
}

struct InferArgs {
    const float *xyz, *points;
    const int32_t *centre, *idx;
    const unsigned short *w[3];
    const float *b[3];
    float *new_xyz, *out;
    int N, S, K, D, G;   // G = B * S neighbourhoods
    int Kd0, C0, C1, C2;
    int ldA, ldB;
    int group_all;
    int c2_per_wg;       // columns of the last layer this workgroup's blockIdx.y owns
};

// One layer of the tile.  The (row block, column block) units go round-robin over the 4 waves; a wave works NJ <= 2 column blocks of
// one row block at a time.  C/D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// Not LAST: relu(acc + b') is split into its three bf16 pieces here, once, and stored as the next layer's operand planes.
// LAST: max over the K rows of each group instead of the store (x -> relu(x + b') is monotone, so it is applied after the max).
template <int TM, bool LAST, int NJ>
__device__ __forceinline__ void infer_unit(const unsigned short *__restrict__ actIn, int ldin, size_t inplane, int Kd,
                                           const unsigned short *__restrict__ W, size_t wplane, const float *__restrict__ bias, int rb, int col0,
                                           int colstep, unsigned short *__restrict__ actOut, int ldout, size_t outplane, const InferArgs &P) {
    f32x16 acc[NJ], accl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f, accl[j][i] = 0.f;
    infer_chunk<NJ>(actIn + (size_t)rb * 32 * ldin, ldin, inplane, Kd, W, wplane, col0, colstep, acc, accl);
    const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] += accl[j][i];
        const int col = col0 + j * colstep + r;
        const float bc = bias[col];
        if (!LAST) {
#pragma unroll
            for (int i = 0; i < 16; i += 2) {   // registers i and i + 1 are rows `row` and `row + 1`
                const int row = rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                unsigned ph, pm, pl;
                sp_split2(fmaxf(acc[j][i] + bc, 0.f), fmaxf(acc[j][i + 1] + bc, 0.f), ph, pm, pl);
                unsigned short *o = actOut + (size_t)row * ldout + col;
                o[0] = (unsigned short)ph, o[ldout] = (unsigned short)(ph >> 16);
                o[outplane] = (unsigned short)pm, o[outplane + ldout] = (unsigned short)(pm >> 16);
                o[2 * outplane] = (unsigned short)pl, o[2 * outplane + ldout] = (unsigned short)(pl >> 16);
            }
        } else {
            float m0 = acc[j][0], m1 = acc[j][8];   // rows 0..15 live in registers 0..7, rows 16..31 in 8..15
#pragma unroll
            for (int i = 1; i < 8; ++i) m0 = fmaxf(m0, acc[j][i]), m1 = fmaxf(m1, acc[j][8 + i]);
            m0 = fmaxf(m0, __shfl_xor(m0, 32, 64));
            m1 = fmaxf(m1, __shfl_xor(m1, 32, 64));
            const long long row0 = (long long)blockIdx.x * TM + rb * 32;
            if (h == 0) {
                if (P.K == 32) {
                    const long long g = row0 / 32;
                    if (g < P.G) P.out[(size_t)g * P.C2 + col] = fmaxf(fmaxf(m0, m1) + bc, 0.f);
                } else {   // K == 16
                    const long long g = row0 / 16;
                    if (g < P.G) P.out[(size_t)g * P.C2 + col] = fmaxf(m0 + bc, 0.f);
                    if (g + 1 < P.G) P.out[(size_t)(g + 1) * P.C2 + col] = fmaxf(m1 + bc, 0.f);
                }
            }
        }
    }
}

template <int TM, bool LAST>
__device__ __forceinline__ void infer_layer(const unsigned short *__restrict__ actIn, int ldin, size_t inplane, int Kd,
                                            const unsigned short *__restrict__ W, int Cout, const float *__restrict__ bias, int colbeg, int ncb,
                                            unsigned short *__restrict__ actOut, int ldout, size_t outplane, const InferArgs &P) {
    constexpr int NRB = TM / 32, WPR = 4 / NRB;   // row blocks; waves per row block
    const size_t wplane = (size_t)Cout * Kd;
    const int wave = threadIdx.x >> 6;
    const int rb = wave % NRB;
    int jb = wave / NRB;
    while (jb < ncb) {   // wave-uniform
        const int left = (ncb - jb + WPR - 1) / WPR;
        const int col0 = colbeg + jb * 32;
        if (left >= 2) {
            infer_unit<TM, LAST, 2>(actIn, ldin, inplane, Kd, W, wplane, bias, rb, col0, 32 * WPR, actOut, ldout, outplane, P);
            jb += 2 * WPR;
        } else {
            infer_unit<TM, LAST, 1>(actIn, ldin, inplane, Kd, W, wplane, bias, rb, col0, 32 * WPR, actOut, ldout, outplane, P);
            jb += WPR;
        }
    }
}

// Rows [m0, m0 + nrows) of the level's G * K grouped rows as the layer-0 operand [xyz[nbr] - xyz[centre] | points[nbr] | 0], split
// as it is written into the three planes of bufA: 16 lanes per row.  Rows past M are zeros.
__device__ __forceinline__ void infer_stage_rows(const InferArgs &P, unsigned short *__restrict__ bufA, size_t planeA, int nrows, long long m0,
                                                 long long M) {
    const int t = threadIdx.x;
    for (int row = t >> 4; row < nrows; row += kInferThreads / 16) {
        const long long m = m0 + row;
        unsigned short *dst = bufA + (size_t)row * P.ldA;
        const int lane = t & 15;
        const bool valid = m < M;
        size_t src = 0, ctr = 0;
        if (valid) {
            const long long g = m / P.K;
            const int b = (int)(g / P.S);
            if (P.group_all) {
                src = (size_t)b * P.N + (int)(m % P.K);
            } else {
                src = (size_t)b * P.N + min(max(P.idx[m], 0), P.N - 1);
                ctr = (size_t)b * P.N + min(max(P.centre[g], 0), P.N - 1);
            }
        }
        for (int c = lane; c < P.Kd0; c += 16) {
            float v = 0.f;
            if (valid) {
                if (c < 3) {
                    v = P.xyz[src * 3 + c];
                    if (!P.group_all) v -= P.xyz[ctr * 3 + c];
                } else if (c < 3 + P.D) {
                    v = P.points[src * P.D + (c - 3)];
                }
            }
            unsigned ph, pm, pl;
            sp_split2(v, 0.f, ph, pm, pl);
            dst[c] = (unsigned short)ph, dst[planeA + c] = (unsigned short)pm, dst[2 * planeA + c] = (unsigned short)pl;
        }
    }
}

template <int TM>
__global__ __launch_bounds__(kInferThreads) void sa_infer_kernel(const InferArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
    const size_t planeA = (size_t)TM * P.ldA, planeB = (size_t)TM * P.ldB;
    unsigned short *bufA = lds;               // three planes of the layer-0 operand, later of layer 1's output (row stride ldA)
    unsigned short *bufB = lds + 3 * planeA;  // three planes of layer 0's output (row stride ldB)
    const int t = threadIdx.x;
    const long long M = (long long)P.G * P.K;
    const long long tile0 = (long long)blockIdx.x * TM;

    // centres of this tile's groups (pointnet_pp_8dir.py:24 / :29): zeros for group_all, the gathered rows otherwise
    if (blockIdx.y == 0 && t < (TM / 16) * 3) {
        const int ngrp = TM / P.K;
        const long long g = tile0 / P.K + t / 3;
        if (t / 3 < ngrp && g < P.G) {
            float v = 0.f;
            if (!P.group_all) {
                const int b = (int)(g / P.S);
                const int c = min(max(P.centre[g], 0), P.N - 1);
                v = P.xyz[((size_t)b * P.N + c) * 3 + t % 3];
            }
            P.new_xyz[g * 3 + t % 3] = v;
        }
    }

    // 1. layer-0 operand, split as it is written
    infer_stage_rows(P, bufA, planeA, TM, tile0, M);
    __syncthreads();
    // 2. the three products
    infer_layer<TM, false>(bufA, P.ldA, planeA, P.Kd0, P.w[0], P.C0, P.b[0], 0, P.C0 / 32, bufB, P.ldB, planeB, P);
    __syncthreads();
    infer_layer<TM, false>(bufB, P.ldB, planeB, P.C0, P.w[1], P.C1, P.b[1], 0, P.C1 / 32, bufA, P.ldA, planeA, P);
    __syncthreads();
    infer_layer<TM, true>(bufA, P.ldA, planeA, P.C1, P.w[2], P.C2, P.b[2], blockIdx.y * P.c2_per_wg, P.c2_per_wg / 32, nullptr, 0, 0, P);
}

// The last layer of one 32-row tile for the wide kernel: the tile's column maxima of z = act W^T (bias and ReLU come after the max over
// the whole neighbourhood, x -> relu(x + b') being monotone) folded into mx[j], the running maxima of NJ column blocks.
template <int NJ>
__device__ __forceinline__ void infer_unit_max(const unsigned short *__restrict__ actIn, int ldin, size_t inplane, int Kd,
                                               const unsigned short *__restrict__ W, size_t wplane, int col0, int colstep, float (&mx)[NJ]) {
    f32x16 acc[NJ], accl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f, accl[j][i] = 0.f;
    infer_chunk<NJ>(actIn, ldin, inplane, Kd, W, wplane, col0, colstep, acc, accl);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        float m = acc[j][0] + accl[j][0];
#pragma unroll
        for (int i = 1; i < 16; ++i) m = fmaxf(m, acc[j][i] + accl[j][i]);
        mx[j] = fmaxf(mx[j], fmaxf(m, __shfl_xor(m, 32, 64)));   // the other half-wave holds the column's other 16 rows
    }
}

// K = 32 m rows per neighbourhood: workgroup blockIdx.x owns neighbourhood g = blockIdx.x, every tile is full.  The column blocks of
// the last layer go round-robin over the 4 waves as in infer_layer<32, true> (a wave works blocks jb and jb + 4 together, then
// jb + 8 ...): at most 32 / 4 = 8 blocks per wave, so a lane's running maxima are 8 registers, indexed statically.
__global__ __launch_bounds__(kInferThreads) void sa_infer_wide_kernel(const InferArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
    const size_t planeA = (size_t)32 * P.ldA, planeB = (size_t)32 * P.ldB;
    unsigned short *bufA = lds;
    unsigned short *bufB = lds + 3 * planeA;
    const int t = threadIdx.x, wave = t >> 6;
    const long long g = blockIdx.x;
    const long long M = (long long)P.G * P.K;

    if (blockIdx.y == 0 && t < 3) {   // the centre (zeros for group_all)
        float v = 0.f;
        if (!P.group_all) {
            const int b = (int)(g / P.S);
            const int c = min(max(P.centre[g], 0), P.N - 1);
            v = P.xyz[((size_t)b * P.N + c) * 3 + t];
        }
        P.new_xyz[g * 3 + t] = v;
    }

    const int colbeg = blockIdx.y * P.c2_per_wg, ncb = P.c2_per_wg / 32;
    const size_t wplane2 = (size_t)P.C2 * P.C1;
    float runmax[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) runmax[i] = -INFINITY;

    for (int tile = 0; tile < P.K / 32; ++tile) {
        infer_stage_rows(P, bufA, planeA, 32, g * P.K + tile * 32, M);
        __syncthreads();
        infer_layer<32, false>(bufA, P.ldA, planeA, P.Kd0, P.w[0], P.C0, P.b[0], 0, P.C0 / 32, bufB, P.ldB, planeB, P);
        __syncthreads();
        infer_layer<32, false>(bufB, P.ldB, planeB, P.C0, P.w[1], P.C1, P.b[1], 0, P.C1 / 32, bufA, P.ldA, planeA, P);
        __syncthreads();
        // one copy of the product code: the loop is not unrolled, the unit at hand is always runmax[0 .. 1] and the array is rotated
        // by two per step (four steps bring it back), so no register is indexed dynamically
#pragma unroll 1
        for (int u = 0; u < 4; ++u) {
            const int jb = wave + 8 * u;   // wave-uniform
            float mx[2] = {runmax[0], runmax[1]};
            if (jb + 4 < ncb) {
                infer_unit_max<2>(bufA, P.ldA, planeA, P.C1, P.w[2], wplane2, colbeg + jb * 32, 128, mx);
            } else if (jb < ncb) {
                float m1[1] = {mx[0]};
                infer_unit_max<1>(bufA, P.ldA, planeA, P.C1, P.w[2], wplane2, colbeg + jb * 32, 128, m1);
                mx[0] = m1[0];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) runmax[i] = runmax[i + 2];
            runmax[6] = mx[0], runmax[7] = mx[1];
        }
        __syncthreads();   // the next tile's operand overwrites bufA
    }

    if (((t >> 5) & 1) == 0) {
        const int r = t & 31;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jb = wave + 8 * u;
            if (jb >= ncb) continue;
            const int col = colbeg + jb * 32 + r;
            P.out[(size_t)g * P.C2 + col] = fmaxf(runmax[2 * u] + P.b[2][col], 0.f);
            if (jb + 4 < ncb) P.out[(size_t)g * P.C2 + col + 128] = fmaxf(runmax[2 * u + 1] + P.b[2][col + 128], 0.f);
        }
    }
}

}  // namespace

int sa_infer_supported(const pnpp_sa_desc *d) {
    InferPlan p;
    return infer_plan(d, &p) == PNPP_OK ? 1 : 0;
}

size_t sa_infer_weights_bytes(const pnpp_sa_desc *d) {
    InferPlan p;
    if (infer_plan(d, &p) != PNPP_OK) return 0;
    return infer_blob(d, p, nullptr).bytes;
}

int sa_infer_weights_layout(const pnpp_sa_desc *d, int layer, size_t *w_offset, int *w_ld, size_t *b_offset) {
    InferPlan p;
    int rc = infer_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(layer >= 0 && layer < 3 && w_offset && w_ld && b_offset, PNPP_ERR_ARG, "sa_infer_weights_layout: layer %d out of range or null pointer", layer);
    const InferBlob b = infer_blob(d, p, nullptr);
    *w_offset = b.woff[layer];
    *b_offset = b.boff[layer];
    *w_ld = b.ld[layer];
    return PNPP_OK;
}

int launch_bn_fold(const float *w, int Cin, const float *b, const float *gamma, const float *beta, const float *rm, const float *rv, float eps,
                   int C, int ld, float *wout, float *bout, hipStream_t st) {
    ProfScope ps(st, "bn_fold_kernel C=%d Cin=%d", C, Cin);
    hipLaunchKernelGGL(bn_fold_kernel, dim3(C), dim3(256), 0, st, w, Cin, b, gamma, beta, rm, rv, eps, ld, wout, bout);
    PNPP_CHECK_LAUNCH("bn_fold");
    return PNPP_OK;
}

int launch_bn_fold_split(const float *w, int Cin, const float *b, const float *gamma, const float *beta, const float *rm, const float *rv,
                                float eps, int C, int ld, unsigned short *wout, float *bout, hipStream_t st) {
    ProfScope ps(st, "bn_fold_split_kernel C=%d Cin=%d", C, Cin);
    hipLaunchKernelGGL(bn_fold_split_kernel, dim3(C), dim3(256), 0, st, w, Cin, b, gamma, beta, rm, rv, eps, ld, wout, bout);
    PNPP_CHECK_LAUNCH("bn_fold_split");
    return PNPP_OK;
}

int sa_infer_fold(const pnpp_sa_desc *d, const pnpp_sa_fwd_args *a, void *weights, hipStream_t st) {
    InferPlan p;
    int rc = infer_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(a && weights, PNPP_ERR_ARG, "sa_infer_fold: null pointer");
    for (int l = 0; l < 3; ++l)
        PNPP_REQUIRE(a->conv_w[l] && a->conv_b[l] && a->bn_w[l] && a->bn_b[l] && a->bn_rm[l] && a->bn_rv[l], PNPP_ERR_ARG,
                     "sa_infer_fold: null parameter pointer in layer %d", l);
    const InferBlob bl = infer_blob(d, p, weights);
    for (int l = 0; l < 3; ++l) {
        rc = launch_bn_fold_split(a->conv_w[l], l == 0 ? d->D + 3 : d->C[l - 1], a->conv_b[l], a->bn_w[l], a->bn_b[l], a->bn_rm[l], a->bn_rv[l],
                                  d->eps, d->C[l], bl.ld[l], bl.w[l], bl.b[l], st);
        if (rc != PNPP_OK) return rc;
    }
    return PNPP_OK;
}

int sa_infer(const pnpp_sa_desc *d, const pnpp_sa_infer_args *a, hipStream_t st) {
    PNPP_REQUIRE(d && a, PNPP_ERR_ARG, "sa_infer: null pointer");
    PNPP_REQUIRE(a->xyz && a->weights && a->new_xyz && a->out, PNPP_ERR_ARG, "sa_infer: null pointer");
    InferPlan p;
    int rc = infer_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(d->D == 0 || a->points, PNPP_ERR_ARG, "sa_infer: D=%d but points is null", d->D);
    const int32_t *idx = nullptr;
    if (!d->group_all) {
        PNPP_REQUIRE(a->centre_idx, PNPP_ERR_ARG, "sa_infer: centre_idx is null");
        PNPP_REQUIRE(a->neighbour_idx || a->idx_out, PNPP_ERR_ARG, "sa_infer: neither neighbour_idx nor idx_out is given");
        PNPP_REQUIRE(d->S <= d->N, PNPP_ERR_RANGE, "sa_infer: npoint=%d > N=%d", d->S, d->N);
        idx = a->neighbour_idx;
        if (!idx) {   // the level searches its own neighbours (pointnet_pp_8dir.py:29-30)
            rc = launch_knn_centres(a->xyz, a->centre_idx, d->B, d->S, d->N, d->K, a->idx_out, a->new_xyz, nullptr, st);
            if (rc != PNPP_OK) return rc;
            idx = a->idx_out;
        }
    }
    const InferBlob bl = infer_blob(d, p, const_cast<void *>(a->weights));
    InferArgs P;
    P.xyz = a->xyz, P.points = a->points, P.centre = a->centre_idx, P.idx = idx;
    for (int l = 0; l < 3; ++l) P.w[l] = bl.w[l], P.b[l] = bl.b[l];
    P.new_xyz = a->new_xyz, P.out = a->out;
    P.N = d->N, P.S = d->S, P.K = d->K, P.D = d->D, P.G = d->B * d->S;
    P.Kd0 = p.Kd0, P.C0 = d->C[0], P.C1 = d->C[1], P.C2 = d->C[2];
    P.ldA = p.ldA, P.ldB = p.ldB;
    P.group_all = d->group_all;
    P.c2_per_wg = d->C[2] / p.nsplit;
    ProfScope ps(st, "%s TM=%d G=%d K=%d D=%d C=%d,%d,%d split=%d", p.wide ? "sa_infer_wide_kernel" : "sa_infer_kernel", p.TM, P.G, d->K, d->D,
                 d->C[0], d->C[1], d->C[2], p.nsplit);
    const dim3 grid(p.ntiles, p.nsplit);
    // dynamic LDS above 48 KiB has to be allowed once per kernel (process-wide flag, not per device: one process drives one GPU)
    static bool granted[3] = {false, false, false};
    const int ki = p.wide ? 2 : p.TM == 64 ? 0 : 1;
    if (p.lds > 48 * 1024 && !granted[ki]) {
        const void *fn = ki == 2 ? (const void *)sa_infer_wide_kernel : ki == 0 ? (const void *)sa_infer_kernel<64> : (const void *)sa_infer_kernel<32>;
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kInferMaxLds);
        PNPP_REQUIRE(e == hipSuccess, PNPP_ERR_LAUNCH, "sa_infer: cannot allow %d bytes of dynamic LDS: %s", kInferMaxLds, hipGetErrorString(e));
        granted[ki] = true;
    }
    if (p.wide)
        hipLaunchKernelGGL(sa_infer_wide_kernel, grid, dim3(kInferThreads), p.lds, st, P);
    else if (p.TM == 64)
        hipLaunchKernelGGL(sa_infer_kernel<64>, grid, dim3(kInferThreads), p.lds, st, P);
    else
        hipLaunchKernelGGL(sa_infer_kernel<32>, grid, dim3(kInferThreads), p.lds, st, P);
    PNPP_CHECK_LAUNCH("sa_infer");
    return PNPP_OK;
}

}  // namespace pnpp

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace pnpp;

extern "C" int pnpp_sa_infer_supported(const pnpp_sa_desc *d) { return sa_infer_supported(d); }
extern "C" size_t pnpp_sa_infer_weights_bytes(const pnpp_sa_desc *d) { return sa_infer_weights_bytes(d); }
extern "C" int pnpp_sa_infer_weights_layout(const pnpp_sa_desc *d, int layer, size_t *w_offset_host, int *w_ld_host, size_t *b_offset_host) {
    return sa_infer_weights_layout(d, layer, w_offset_host, w_ld_host, b_offset_host);
}
extern "C" int pnpp_sa_infer_fold(const pnpp_sa_desc *d, const pnpp_sa_fwd_args *params, void *weights, void *stream) {
    return sa_infer_fold(d, params, weights, as_stream(stream));
}
extern "C" int pnpp_sa_infer(const pnpp_sa_desc *d, const pnpp_sa_infer_args *a, void *stream) { return sa_infer(d, a, as_stream(stream)); }
static int sa_infer_group_pair_impl(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *lengths,
                                    const int32_t *centre1, const int32_t *centre2, int32_t *idx1, float *new_xyz1, int32_t *idx2,
                                    float *new_xyz2, void *stream) {
    PNPP_REQUIRE(d1 && d2, PNPP_ERR_ARG, "sa_infer_group_pair: null descriptor");
    PNPP_REQUIRE(!d1->group_all && !d2->group_all, PNPP_ERR_ARG, "sa_infer_group_pair: both levels must group neighbourhoods");
    PNPP_REQUIRE(d1->B == d2->B && d2->N == d1->S, PNPP_ERR_ARG, "sa_infer_group_pair: level 2 must take level 1's %d centres (got N=%d)", d1->S,
                 d2->N);
    PNPP_REQUIRE(xyz && centre1 && centre2 && idx1 && idx2 && new_xyz1 && new_xyz2, PNPP_ERR_ARG, "sa_infer_group_pair: null pointer");
    return launch_knn_pair(xyz, d1->B, d1->N, centre1, d1->S, d1->K, idx1, new_xyz1, nullptr, centre2, d2->S, d2->K, idx2, new_xyz2, nullptr, nullptr,
                           as_stream(stream), lengths);
}
extern "C" int pnpp_sa_infer_group_pair(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *centre1,
                                        const int32_t *centre2, int32_t *idx1, float *new_xyz1, int32_t *idx2, float *new_xyz2, void *stream) {
    return sa_infer_group_pair_impl(d1, d2, xyz, nullptr, centre1, centre2, idx1, new_xyz1, idx2, new_xyz2, stream);
}
extern "C" int pnpp_sa_infer_group_pair_ragged(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *lengths,
                                               const int32_t *centre1, const int32_t *centre2, int32_t *idx1, float *new_xyz1, int32_t *idx2,
                                               float *new_xyz2, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "sa_infer_group_pair_ragged: null lengths");
    return sa_infer_group_pair_impl(d1, d2, xyz, lengths, centre1, centre2, idx1, new_xyz1, idx2, new_xyz2, stream);
}
extern "C" int pnpp_fc_infer_fold(int N, int K, const float *w, const float *b, const float *gamma, const float *beta, const float *rm,
                                  const float *rv, float eps, float *w_out, float *b_out, void *stream) {
    PNPP_REQUIRE(N > 0 && K > 0, PNPP_ERR_ARG, "fc_infer_fold: non-positive size N=%d K=%d", N, K);
    PNPP_REQUIRE(w && b && gamma && beta && rm && rv && w_out && b_out, PNPP_ERR_ARG, "fc_infer_fold: null pointer");
    return launch_bn_fold(w, K, b, gamma, beta, rm, rv, eps, N, K, w_out, b_out, as_stream(stream));
}
