// pointnet_infer_kernels.hip -- forward-only (inference) path of a vanilla PointNet trunk: one launch per trunk + a small finishing pass.
//
// Reference: models/pointnet.py (STN3d / STNkd / PointNetEncoder) evaluated with BatchNorm in eval mode.  Each BatchNorm folds into
// the 1x1 convolution in front of it (launch_bn_fold_split: float64, rounded once, W' stored as three fragment-major bf16 planes), so
// a trunk is   rows -> L x (product + b' [+ ReLU]) -> max over the cloud's N points,
// optionally with the cloud's 3 x 3 transform applied to the first three input columns while the layer-0 operand is built and the
// cloud's 64 x 64 feature transform as a product layer of its own between two layers (no bias, no ReLU; its planes are split per call
// by pn_split_transform_kernel, 24 KiB per cloud).
//
// pn_infer_kernel: a workgroup (4 waves) owns TM consecutive rows of ONE cloud (tiles never straddle clouds).
//   1. builds the layer-0 operand [x[:3] @ trans | x[3:] | 0] in LDS, split into its three bf16 planes as it is written,
//   2. runs the stages with the routines of sa_infer_kernel (split_infer.h: float32 products on v_mfma_f32_32x32x16_bf16 from exact
//      three-way splits, leading and small products in separate accumulators), handing each stage's output tile to the next through
//      two LDS tiles used alternately; an activation is split once, by the lane that produced it,
//   3. takes the max over each 32-row block's valid rows from the last layer's accumulators and writes one partial row per
//      (cloud, 32-row block): part (B, ceil(N/32), C_last).  Rows beyond N are left out of the max.
// pn_infer_finish_kernel: out[b][c] = act(max over the cloud's partial rows + b'[c]) -- x -> act(x + b') is monotone, and the folded
// W' carries the sign of gamma / sqrt(var + eps), so a plain max is right for negative gamma too.
// Nothing of size B*N x C is written for C > 64; no atomics, no workgroup reads what another workgroup of the same launch wrote, so
// results are bitwise identical from call to call.  When B * tiles is below the CU count the last layer's columns are split over
// blockIdx.y and every such workgroup recomputes the narrow stages of its tile.
//
// Shapes taken (pnpp_pn_infer_supported): L = 2 .. 4; C[l] multiples of 32, <= 1024; 1 <= D <= 1024; transform_after only behind a
// 64-wide layer; the two LDS tiles of a 32-row workgroup fit 160 KiB; any B, N >= 1 within int32 sizes.
#include "kernels.h"
#include "split_infer.h"

namespace pnpp {

namespace {

constexpr int kPnThreads = 256;
constexpr int kPnMaxLds = 160 * 1024;
constexpr int kPnMaxStages = PNPP_MAX_LAYERS + 1;
constexpr int kPnK = 64;   // the feature transform's size

struct PnPlan {
    int TM;                   // rows per workgroup (32 or 64)
    int Kd0;                  // layer 0's reduction length, padded to a multiple of 16
    int ldA, ldB;             // row strides of the two LDS tiles (bf16 elements)
    int nstage;               // layers + the feature transform
    int layer[kPnMaxStages];  // stage -> layer, -1 for the feature transform
    int kin[kPnMaxStages], cout[kPnMaxStages];
    int tiles, nslot;         // row tiles and 32-row blocks per cloud
    int nsplit;               // column split of the last layer over blockIdx.y
    size_t lds, part_bytes, scratch_bytes;
};

struct PnBlob {
    unsigned short *w[PNPP_MAX_LAYERS];
    float *b[PNPP_MAX_LAYERS];
    size_t woff[PNPP_MAX_LAYERS], boff[PNPP_MAX_LAYERS];   // as InferBlob of sa_infer_kernels.hip, 256-byte aligned
    int ld[PNPP_MAX_LAYERS];
    size_t bytes;
};

static int pn_plan(const pnpp_pn_infer_desc *d, PnPlan *p) {
    PNPP_REQUIRE(d, PNPP_ERR_ARG, "pn_infer: null descriptor");
    PNPP_REQUIRE(d->B > 0 && d->N > 0 && d->D > 0, PNPP_ERR_ARG, "pn_infer: bad geometry B=%d N=%d D=%d", d->B, d->N, d->D);
    PNPP_REQUIRE(d->L >= 2 && d->L <= PNPP_MAX_LAYERS, PNPP_ERR_ARG, "pn_infer: the fused kernel takes 2 to %d layers, not %d", PNPP_MAX_LAYERS,
                 d->L);
    for (int l = 0; l < d->L; ++l)
        PNPP_REQUIRE(d->C[l] > 0 && d->C[l] % 32 == 0 && d->C[l] <= 1024, PNPP_ERR_ARG,
                     "pn_infer: layer width %d (=%d) must be a multiple of 32 up to 1024", l, d->C[l]);
    PNPP_REQUIRE(d->D <= 1024, PNPP_ERR_ARG, "pn_infer: D=%d input channels exceed 1024", d->D);
    PNPP_REQUIRE(!d->input_transform || d->D >= 3, PNPP_ERR_ARG, "pn_infer: the 3 x 3 input transform needs D >= 3, not D=%d", d->D);
    PNPP_REQUIRE(d->transform_after >= -1 && d->transform_after < d->L - 1, PNPP_ERR_ARG,
                 "pn_infer: transform_after=%d is not a layer in front of the pooled one", d->transform_after);
    if (d->transform_after >= 0)
        PNPP_REQUIRE(d->C[d->transform_after] == kPnK, PNPP_ERR_ARG, "pn_infer: the feature transform is %d x %d, layer %d is %d wide", kPnK,
                     kPnK, d->transform_after, d->C[d->transform_after]);
    PNPP_REQUIRE((long long)d->B * d->N < (1ll << 31) && (long long)d->B * d->N * d->D < (1ll << 31), PNPP_ERR_ARG,
                 "pn_infer: B*N or B*N*D overflows int32");
    p->Kd0 = (d->D + 15) & ~15;
    int s = 0, width = p->Kd0;
    for (int l = 0; l < d->L; ++l) {
        p->layer[s] = l, p->kin[s] = width, p->cout[s] = d->C[l], width = d->C[l], ++s;
        if (d->transform_after == l) p->layer[s] = -1, p->kin[s] = width, p->cout[s] = width, ++s;
    }
    p->nstage = s;
    int wa = 0, wb = 0;   // stage s reads tile A when s is even, tile B when odd, and writes the other
    for (s = 0; s < p->nstage; ++s) {
        int &wide = (s & 1) ? wb : wa;
        wide = p->kin[s] > wide ? p->kin[s] : wide;
    }
    p->ldA = wa + 8;   // bf16 elements; + 16 bytes: the 32 rows of a 16-byte-per-lane read fall on different banks
    p->ldB = wb + 8;
    const size_t per_row = (size_t)(p->ldA + p->ldB) * 3 * sizeof(unsigned short);
    p->TM = (64 * per_row <= 80 * 1024 && d->N > 32) ? 64 : 32;   // 64 rows when two workgroups per CU still fit
    p->lds = p->TM * per_row;
    PNPP_REQUIRE(p->lds <= (size_t)kPnMaxLds, PNPP_ERR_ARG, "pn_infer: a 32-row tile of widths %d and %d needs %zu bytes of LDS (> %d)", wa, wb,
                 p->lds, kPnMaxLds);
    p->tiles = (d->N + p->TM - 1) / p->TM;
    p->nslot = (d->N + 31) / 32;
    const int clast = d->C[d->L - 1];
    int ns = 1;
    const long long wgs = (long long)d->B * p->tiles;
    const int target = infer_target_wgs();
    while (wgs * ns < target && (clast / 32) % (ns * 2) == 0 && clast / (ns * 2) >= 128) ns *= 2;
    p->nsplit = ns;
    p->part_bytes = align_up((size_t)d->B * p->nslot * clast * sizeof(float), 256);
    p->scratch_bytes = p->part_bytes + (d->transform_after >= 0 ? (size_t)d->B * 3 * kPnK * kPnK * sizeof(unsigned short) : 0);
    return PNPP_OK;
}

static PnBlob pn_blob(const pnpp_pn_infer_desc *d, const PnPlan &p, void *base) {
    PnBlob b;
    size_t off = 0;
    char *cb = static_cast<char *>(base);
    for (int l = 0; l < d->L; ++l) {
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

// The cloud's k x k transform as the weight of a product layer, y = h @ T: W[n][j] = T[j][n], written as the three fragment-major
// bf16 planes of its exact split (the layout of bn_fold_split_kernel with C = ld = k); out + b * 3 k^2
__global__ __launch_bounds__(256) void pn_split_transform_kernel(const float *__restrict__ T, int k, unsigned short *__restrict__ out) {
    const size_t plane = (size_t)k * k;
    const float *t = T + blockIdx.x * plane;
    unsigned short *o = out + blockIdx.x * 3 * plane;
    for (int e = threadIdx.x; e < k * k; e += blockDim.x) {
        const int j = e / k, n = e % k;
        unsigned h, m, l;
        sp_split2(t[e], 0.f, h, m, l);
        const size_t at = ((((size_t)(n >> 5) * (k >> 4) + (j >> 4)) * 64 + (((j & 15) >> 3) << 5) + (n & 31)) << 3) + (j & 7);
        o[at] = (unsigned short)h, o[plane + at] = (unsigned short)m, o[2 * plane + at] = (unsigned short)l;
    }
}

struct PnStage {
    const unsigned short *w;   // three planes of Cout x Kd, fragment-major
    const float *bias;         // Cout, or null (the feature transform)
    long long cloud_stride;    // elements between two clouds' planes (the feature transform), 0 for shared weights
    int Kd, Cout, relu;
};

struct PnArgs {
    const float *x;
    long long sb, sn, sc;
    const float *trans;        // (B,3,3) or null
    PnStage st[kPnMaxStages];
    int nstage;
    float *part;               // (B, nslot, C_last)
    float *feat_out;           // (B*N, Cout[feat_stage]) or null
    int feat_stage;
    int N, D, Kd0;
    int ldA, ldB;
    int tiles, nslot;
    int c_per_wg;              // columns of the last layer this workgroup's blockIdx.y owns
    const int32_t *offs;       // ragged batches: (B + 1) exclusive prefix sums of the lengths (cloud b holds offs[b+1] - offs[b] rows)
};

// One stage of the tile, as infer_unit of sa_infer_kernels.hip.  C/D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// Not LAST: act(acc + b') is split into its three bf16 pieces here, once, and stored as the next stage's operand planes (and, for the
// tapped stage, written as float32 rows to feat_out).  LAST: max over the block's rows n < N instead of the store.
template <bool LAST, int NJ>
__device__ __forceinline__ void pn_unit(const unsigned short *__restrict__ actIn, int ldin, size_t inplane, const PnStage &S,
                                        const unsigned short *__restrict__ W, int rb, int col0, int colstep,
                                        unsigned short *__restrict__ actOut, int ldout, size_t outplane, float *__restrict__ dst, int n0, int N) {
    f32x16 acc[NJ], accl[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f, accl[j][i] = 0.f;
    infer_chunk<NJ>(actIn + (size_t)rb * 32 * ldin, ldin, inplane, S.Kd, W, (size_t)S.Cout * S.Kd, col0, colstep, acc, accl);
    const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
    const int nb = n0 + rb * 32;   // the block's first row in its cloud
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] += accl[j][i];
        const int col = col0 + j * colstep + r;
        if (!LAST) {
            const float bc = S.bias ? S.bias[col] : 0.f;
#pragma unroll
            for (int i = 0; i < 16; i += 2) {   // registers i and i + 1 are rows `row` and `row + 1`
                const int row = rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                float v0 = acc[j][i] + bc, v1 = acc[j][i + 1] + bc;
                if (S.relu) v0 = fmaxf(v0, 0.f), v1 = fmaxf(v1, 0.f);
                unsigned ph, pm, pl;
                sp_split2(v0, v1, ph, pm, pl);
                unsigned short *o = actOut + (size_t)row * ldout + col;
                o[0] = (unsigned short)ph, o[ldout] = (unsigned short)(ph >> 16);
                o[outplane] = (unsigned short)pm, o[outplane + ldout] = (unsigned short)(pm >> 16);
                o[2 * outplane] = (unsigned short)pl, o[2 * outplane + ldout] = (unsigned short)(pl >> 16);
                if (dst) {   // dst = feat_out + (first row of the cloud) * Cout
                    const int n = n0 + row;
                    if (n < N) dst[(size_t)n * S.Cout + col] = v0;
                    if (n + 1 < N) dst[(size_t)(n + 1) * S.Cout + col] = v1;
                }
            }
        } else {
            float m = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int n = nb + (i & 3) + 8 * (i >> 2) + 4 * h;
                m = fmaxf(m, n < N ? acc[j][i] : -INFINITY);
            }
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            if (h == 0) dst[col] = m;   // dst = this block's partial row
        }
    }
}

template <int TM, bool LAST>
__device__ __forceinline__ void pn_layer(const unsigned short *__restrict__ actIn, int ldin, size_t inplane, const PnStage &S,
                                         const unsigned short *__restrict__ W, int colbeg, int ncb, unsigned short *__restrict__ actOut,
                                         int ldout, size_t outplane, float *__restrict__ dst, int n0, int N, int slot_stride) {
    constexpr int NRB = TM / 32, WPR = 4 / NRB;   // row blocks; waves per row block
    const int wave = threadIdx.x >> 6;
    const int rb = wave % NRB;
    if (LAST) {
        if (n0 + rb * 32 >= N) return;   // wave-uniform: a block without a valid row has no partial row (no barrier follows)
        dst += (size_t)rb * slot_stride;
    }
    int jb = wave / NRB;
    while (jb < ncb) {   // wave-uniform
        const int left = (ncb - jb + WPR - 1) / WPR;
        const int col0 = colbeg + jb * 32;
        if (left >= 2) {
            pn_unit<LAST, 2>(actIn, ldin, inplane, S, W, rb, col0, 32 * WPR, actOut, ldout, outplane, dst, n0, N);
            jb += 2 * WPR;
        } else {
            pn_unit<LAST, 1>(actIn, ldin, inplane, S, W, rb, col0, 32 * WPR, actOut, ldout, outplane, dst, n0, N);
            jb += WPR;
        }
    }
}

// RAGGED: the cloud's own row count Nv takes N's place in the operand build, the tapped stores and the max; the input and feat_out keep
// their padded addressing (feat_out rows n >= Nv are written as zeros), and a tile beyond Nv leaves before the first barrier.
template <int TM, bool RAGGED>
__global__ __launch_bounds__(kPnThreads) void pn_infer_kernel(const PnArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
    const size_t planeA = (size_t)TM * P.ldA, planeB = (size_t)TM * P.ldB;
    unsigned short *bufA = lds;               // three planes, row stride ldA: the layer-0 operand, then every odd stage's output
    unsigned short *bufB = lds + 3 * planeA;  // three planes, row stride ldB: every even stage's output
    const int t = threadIdx.x;
    const int b = blockIdx.x / P.tiles;
    const int n0 = (blockIdx.x % P.tiles) * TM;
    int Nv = P.N;
    if (RAGGED) {
        Nv = min(max(P.offs[b + 1] - P.offs[b], 0), P.N);   // wave-uniform loads
        if (P.feat_out && blockIdx.y == 0) {   // the padding rows of this tile in the tapped output
            const int cf = P.st[P.feat_stage].Cout, nz0 = max(n0, Nv), nz1 = min(n0 + TM, P.N);
            float *fz = P.feat_out + ((size_t)b * P.N + nz0) * cf;
            for (int e = t; e < (nz1 - nz0) * cf; e += kPnThreads) fz[e] = 0.f;
        }
        if (n0 >= Nv) return;   // block-uniform
    }

    // 1. layer-0 operand, split as it is written: consecutive threads take consecutive rows of one column
    const float *xb = P.x + (long long)b * P.sb;
    const float *tb = P.trans ? P.trans + (size_t)b * 9 : nullptr;
    for (int e = t; e < TM * P.Kd0; e += kPnThreads) {
        const int row = e % TM, c = e / TM;
        const int n = n0 + row;
        float v = 0.f;
        if (n < Nv && c < P.D) {
            const float *xr = xb + (long long)n * P.sn;
            if (tb && c < 3)
                v = fmaf(xr[2 * P.sc], tb[6 + c], fmaf(xr[P.sc], tb[3 + c], xr[0] * tb[c]));
            else
                v = xr[(long long)c * P.sc];
        }
        unsigned ph, pm, pl;
        sp_split2(v, 0.f, ph, pm, pl);
        unsigned short *dst = bufA + (size_t)row * P.ldA + c;
        dst[0] = (unsigned short)ph, dst[planeA] = (unsigned short)pm, dst[2 * planeA] = (unsigned short)pl;
    }
    __syncthreads();
    // 2. the stages in front of the pooled layer
    const int last = P.nstage - 1;
    for (int s = 0; s < last; ++s) {
        const PnStage &S = P.st[s];
        const bool odd = s & 1;
        float *feat = (s == P.feat_stage && P.feat_out && blockIdx.y == 0) ? P.feat_out + (size_t)b * P.N * S.Cout : nullptr;
        pn_layer<TM, false>(odd ? bufB : bufA, odd ? P.ldB : P.ldA, odd ? planeB : planeA, S, S.w + (long long)b * S.cloud_stride, 0, S.Cout / 32,
                            odd ? bufA : bufB, odd ? P.ldA : P.ldB, odd ? planeA : planeB, feat, n0, Nv, 0);
        __syncthreads();
    }
    // 3. the pooled layer: one partial row per 32-row block
    const PnStage &S = P.st[last];
    const bool odd = last & 1;
    float *part = P.part + ((size_t)b * P.nslot + n0 / 32) * S.Cout;
    pn_layer<TM, true>(odd ? bufB : bufA, odd ? P.ldB : P.ldA, odd ? planeB : planeA, S, S.w + (long long)b * S.cloud_stride,
                       blockIdx.y * P.c_per_wg, P.c_per_wg / 32, nullptr, 0, 0, part, n0, Nv, S.Cout);
}

// out[b][c] = act(max_s part[b][s][c] + b'[c]); offs (ragged batches): only the cloud's ceil(Nv / 32) partial rows were written
__global__ __launch_bounds__(256) void pn_infer_finish_kernel(const float *__restrict__ part, const float *__restrict__ bias,
                                                              const int32_t *__restrict__ offs, int nslot, int C, int relu,
                                                              float *__restrict__ out) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float *p = part + (size_t)blockIdx.x * nslot * C + c;
    const int ns = offs ? min(max((offs[blockIdx.x + 1] - offs[blockIdx.x] + 31) / 32, 1), nslot) : nslot;
    float m = p[0];
    for (int s = 1; s < ns; ++s) m = fmaxf(m, p[(size_t)s * C]);
    m += bias[c];
    out[(size_t)blockIdx.x * C + c] = relu ? fmaxf(m, 0.f) : m;
}

}  // namespace

static int pn_infer_fold(const pnpp_pn_infer_desc *d, const pnpp_sa_fwd_args *a, void *weights, hipStream_t st) {
    PnPlan p;
    int rc = pn_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(a && weights, PNPP_ERR_ARG, "pn_infer_fold: null pointer");
    for (int l = 0; l < d->L; ++l)
        PNPP_REQUIRE(a->conv_w[l] && a->conv_b[l] && a->bn_w[l] && a->bn_b[l] && a->bn_rm[l] && a->bn_rv[l], PNPP_ERR_ARG,
                     "pn_infer_fold: null parameter pointer in layer %d", l);
    const PnBlob bl = pn_blob(d, p, weights);
    for (int l = 0; l < d->L; ++l) {
        rc = launch_bn_fold_split(a->conv_w[l], l == 0 ? d->D : d->C[l - 1], a->conv_b[l], a->bn_w[l], a->bn_b[l], a->bn_rm[l], a->bn_rv[l], d->eps,
                                  d->C[l], bl.ld[l], bl.w[l], bl.b[l], st);
        if (rc != PNPP_OK) return rc;
    }
    return PNPP_OK;
}

static int pn_infer(const pnpp_pn_infer_desc *d, const pnpp_pn_infer_args *a, const int32_t *offs, hipStream_t st) {
    PNPP_REQUIRE(d && a, PNPP_ERR_ARG, "pn_infer: null pointer");
    PNPP_REQUIRE(a->x && a->weights && a->scratch && a->out, PNPP_ERR_ARG, "pn_infer: null pointer");
    PnPlan p;
    int rc = pn_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(!d->input_transform || a->trans, PNPP_ERR_ARG, "pn_infer: input_transform is set but trans is null");
    PNPP_REQUIRE(d->transform_after < 0 || a->trans_feat, PNPP_ERR_ARG, "pn_infer: transform_after=%d but trans_feat is null", d->transform_after);
    PNPP_REQUIRE(a->stride_b >= 0 && a->stride_n >= 0 && a->stride_c >= 0, PNPP_ERR_ARG, "pn_infer: negative input stride");
    if (a->feat_out)
        PNPP_REQUIRE(a->feat_layer >= 0 && a->feat_layer < d->L - 1 && d->C[a->feat_layer] <= 64, PNPP_ERR_ARG,
                     "pn_infer: feat_out taps a layer in front of the pooled one that is at most 64 wide, not layer %d", a->feat_layer);
    const PnBlob bl = pn_blob(d, p, const_cast<void *>(a->weights));
    const int clast = d->C[d->L - 1];
    float *part = static_cast<float *>(a->scratch);
    unsigned short *tplanes = reinterpret_cast<unsigned short *>(static_cast<char *>(a->scratch) + p.part_bytes);
    if (d->transform_after >= 0) {
        ProfScope ps(st, "pn_split_transform_kernel B=%d k=%d", d->B, kPnK);
        hipLaunchKernelGGL(pn_split_transform_kernel, dim3(d->B), dim3(256), 0, st, a->trans_feat, kPnK, tplanes);
        PNPP_CHECK_LAUNCH("pn_split_transform");
    }
    PnArgs P;
    P.x = a->x, P.sb = a->stride_b, P.sn = a->stride_n, P.sc = a->stride_c;
    P.trans = d->input_transform ? a->trans : nullptr;
    P.nstage = p.nstage;
    P.feat_stage = -1;
    for (int s = 0; s < p.nstage; ++s) {
        PnStage &S = P.st[s];
        const int l = p.layer[s];
        S.Kd = p.kin[s], S.Cout = p.cout[s];
        if (l >= 0) {
            S.w = bl.w[l], S.bias = bl.b[l], S.cloud_stride = 0;
            S.relu = l < d->L - 1 ? 1 : 0;   // the pooled layer's activation is the finishing pass's
            if (a->feat_out && a->feat_layer == l) P.feat_stage = s;
        } else {
            S.w = tplanes, S.bias = nullptr, S.cloud_stride = 3ll * kPnK * kPnK, S.relu = 0;
            if (a->feat_out && a->feat_layer == d->transform_after) P.feat_stage = s;   // the transformed rows
        }
    }
    for (int s = p.nstage; s < kPnMaxStages; ++s) P.st[s] = PnStage{nullptr, nullptr, 0, 0, 0, 0};
    P.part = part, P.feat_out = a->feat_out;
    P.N = d->N, P.D = d->D, P.Kd0 = p.Kd0;
    P.ldA = p.ldA, P.ldB = p.ldB;
    P.tiles = p.tiles, P.nslot = p.nslot;
    P.c_per_wg = clast / p.nsplit;
    P.offs = offs;
    {
        ProfScope ps(st, "pn_infer_kernel TM=%d B=%d N=%d D=%d L=%d C=%d,%d,%d,%d t3=%d tk=%d split=%d", p.TM, d->B, d->N, d->D, d->L, d->C[0],
                     d->C[1], d->L > 2 ? d->C[2] : 0, d->L > 3 ? d->C[3] : 0, d->input_transform, d->transform_after, p.nsplit);
        const dim3 grid(d->B * p.tiles, p.nsplit);
        // dynamic LDS above 48 KiB has to be allowed once per kernel (process-wide flag, not per device: one process drives one GPU)
        static bool granted[4] = {false, false, false, false};
        const int ki = (p.TM == 64 ? 0 : 1) + (offs ? 2 : 0);
        if (p.lds > 48 * 1024 && !granted[ki]) {
            const void *fns[4] = {(const void *)pn_infer_kernel<64, false>, (const void *)pn_infer_kernel<32, false>,
                                  (const void *)pn_infer_kernel<64, true>, (const void *)pn_infer_kernel<32, true>};
            const void *fn = fns[ki];
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kPnMaxLds);
            PNPP_REQUIRE(e == hipSuccess, PNPP_ERR_LAUNCH, "pn_infer: cannot allow %d bytes of dynamic LDS: %s", kPnMaxLds, hipGetErrorString(e));
            granted[ki] = true;
        }
        if (p.TM == 64 && !offs)
            hipLaunchKernelGGL((pn_infer_kernel<64, false>), grid, dim3(kPnThreads), p.lds, st, P);
        else if (!offs)
            hipLaunchKernelGGL((pn_infer_kernel<32, false>), grid, dim3(kPnThreads), p.lds, st, P);
        else if (p.TM == 64)
            hipLaunchKernelGGL((pn_infer_kernel<64, true>), grid, dim3(kPnThreads), p.lds, st, P);
        else
            hipLaunchKernelGGL((pn_infer_kernel<32, true>), grid, dim3(kPnThreads), p.lds, st, P);
        PNPP_CHECK_LAUNCH("pn_infer");
    }
    {
        ProfScope ps(st, "pn_infer_finish_kernel B=%d slots=%d C=%d relu=%d", d->B, p.nslot, clast, d->relu_last);
        hipLaunchKernelGGL(pn_infer_finish_kernel, dim3(d->B, (clast + 255) / 256), dim3(256), 0, st, part, bl.b[d->L - 1], offs, p.nslot, clast,
                           d->relu_last, a->out);
        PNPP_CHECK_LAUNCH("pn_infer_finish");
    }
    return PNPP_OK;
}

}  // namespace pnpp

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace pnpp;

extern "C" int pnpp_pn_infer_supported(const pnpp_pn_infer_desc *d) {
    PnPlan p;
    return pn_plan(d, &p) == PNPP_OK ? 1 : 0;
}
extern "C" size_t pnpp_pn_infer_weights_bytes(const pnpp_pn_infer_desc *d) {
    PnPlan p;
    if (pn_plan(d, &p) != PNPP_OK) return 0;
    return pn_blob(d, p, nullptr).bytes;
}
extern "C" size_t pnpp_pn_infer_scratch_bytes(const pnpp_pn_infer_desc *d) {
    PnPlan p;
    if (pn_plan(d, &p) != PNPP_OK) return 0;
    return p.scratch_bytes;
}
extern "C" int pnpp_pn_infer_weights_layout(const pnpp_pn_infer_desc *d, int layer, size_t *w_offset_host, int *w_ld_host, size_t *b_offset_host) {
    PnPlan p;
    int rc = pn_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(layer >= 0 && layer < d->L && w_offset_host && w_ld_host && b_offset_host, PNPP_ERR_ARG,
                 "pn_infer_weights_layout: layer %d out of range or null pointer", layer);
    const PnBlob b = pn_blob(d, p, nullptr);
    *w_offset_host = b.woff[layer];
    *b_offset_host = b.boff[layer];
    *w_ld_host = b.ld[layer];
    return PNPP_OK;
}
extern "C" int pnpp_pn_infer_fold(const pnpp_pn_infer_desc *d, const pnpp_sa_fwd_args *params, void *weights, void *stream) {
    return pn_infer_fold(d, params, weights, as_stream(stream));
}
extern "C" int pnpp_pn_infer(const pnpp_pn_infer_desc *d, const pnpp_pn_infer_args *a, void *stream) {
    return pn_infer(d, a, nullptr, as_stream(stream));
}
extern "C" int pnpp_pn_infer_ragged(const pnpp_pn_infer_desc *d, const pnpp_pn_infer_args *a, const int32_t *offs, void *stream) {
    PNPP_REQUIRE(offs, PNPP_ERR_ARG, "pn_infer_ragged: null offsets");
    return pn_infer(d, a, offs, as_stream(stream));
}
