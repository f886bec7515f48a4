// transformer_infer_kernels.hip -- forward-only (inference) path of the point transformer (models/point_transformer.py in eval mode):
// everything of an encoder layer behind the attention is row-local and runs as ONE launch per layer.
//
//   pt_head_infer_kernel   x0 = xyz W_p^T + b_p (K = in_dim <= 8, plain FMA; rows >= n_valid are zero points, padded on the fly) and
//                          qkv_0 = x0 W_in^T + b_in of layer 0
//   pt_tail_infer_kernel   u = LN1(x + o W_out^T + b_out);  h = relu(u W_1^T + b_1);  y = LN2(u + h W_2^T + b_2) -> x_next;  then either
//                          qkv_next = y W_in'^T + b_in' (the NEXT layer's in_proj) or, in the last layer, the column sums of y over each
//                          32-row block's rows n < n_valid
//   pt_pool_infer_kernel   adds a cloud's partial sums in a fixed order, divides by n_valid, applies fc_out
// The attention between two of them stays pnpp_attention_fwd (lse = NULL): 1 + depth * 2 + 1 launches per forward.
// Ragged form (the _ragged entry points): n_valid becomes the cloud's own length in the head's zero-point rule, in the last layer's
// pooling and in the divisor.  No block is skipped: every row of x_next / qkv_next is written on every call, finite, because the
// attention stages keys 64 rows at a time and multiplies what lies beyond the cloud by zero weights -- a stale NaN there would spread.
//
// Products: split_infer.h (float32 products on v_mfma_f32_32x32x16_bf16 from exact three-way splits, leading and small products in
// separate accumulators).  The weights' planes are written once by pnpp_pt_infer_fold, an activation is split once, by the lane that
// produced it.
//
// Tiling of pt_tail_infer_kernel: a workgroup (4 waves) owns 128 consecutive rows of one cloud (N % 128 == 0), a wave its own 32 of
// them from the first load to the last store -- nothing a wave writes to LDS is read by another wave except the weight chunk.  The
// F hidden columns are produced and consumed 64 at a time: the chunk's W_1 rows and W_2 columns (3 planes each, 48 KiB together) are
// staged in LDS ONCE PER WORKGROUP, so one weight fetch from L2 feeds four row tiles (every wave streaming its own copy from L2 would
// move F/64 * 48 KiB = 1.5 MiB per 32 rows); the next chunk's 12 x 16 bytes per thread are in flight in registers while the current
// one is multiplied.  A wave's hidden chunk (32 x 64, three planes) lives in its own LDS tile between the two products and never
// leaves the chip.  W_out and the next in_proj are read once per wave straight from L2 (24 + 72 KiB against 1.5 MiB).
// LDS: 48 KiB weight chunk + 4 x 13.5 KiB u tiles + 4 x 13.5 KiB hidden tiles = 156 KiB (rows are padded by 16 bytes against bank
// conflicts), one workgroup per CU.
// LayerNorm: an accumulator lane holds one column of 16 rows, so a row's statistics are a butterfly over the 32 lanes of a half wave,
// two passes (mean, then centred squares), float32, fixed order.
// No atomics, no workgroup reads what another one of the same launch wrote: results are bitwise identical from call to call.
#include "kernels.h"
#include "split_infer.h"

namespace pnpp {

namespace {

constexpr int kPtThreads = 256;
constexpr int kPtRows = 128;                      // rows per workgroup, 32 per wave
constexpr int kPtE = 64, kPtH = 4;                // the reference model's width and heads
constexpr int kPtChunk = 64;                      // hidden columns per step
constexpr int kPtLd = kPtE + 8;                   // row stride of an LDS tile (bf16 elements; + 16 bytes, as the other inference kernels)
constexpr int kPtPlane = 32 * kPtLd;              // one plane of a wave's tile
constexpr int kPtTile = 3 * kPtPlane;             // a wave's tile: three planes
constexpr int kPtWPlane = kPtChunk * kPtE;        // one plane of a staged weight chunk (64 x 64, fragment-major)
constexpr int kPtWChunk = 2 * 3 * kPtWPlane;      // W_1 rows + W_2 columns of a chunk, three planes each
constexpr int kPtMaxIn = 8;                       // input_proj's reduction length
constexpr size_t kPtTailLds = (size_t)(kPtWChunk + 8 * kPtTile) * sizeof(unsigned short);
constexpr size_t kPtHeadLds = (size_t)(4 * kPtTile) * sizeof(unsigned short);
enum { PT_IN_PROJ = 0, PT_OUT_PROJ = 1, PT_LINEAR1 = 2, PT_LINEAR2 = 3, PT_NORM1 = 4, PT_NORM2 = 5, PT_INPUT_PROJ = 6 };

struct PtPlan {
    int M, tiles32;        // rows, 32-row blocks per cloud
    size_t scratch_bytes;  // the last layer's partial sums (B, N/32, E)
};

// byte offsets inside the blob, all 256-byte aligned
struct PtLayerOff {
    size_t w[4], b[4];     // in_proj, out_proj, linear1, linear2: three fragment-major planes, float32 bias
    size_t g[2], be[2];    // norm1 / norm2 weight and bias
};

static int pt_plan(const pnpp_pt_infer_desc *d, PtPlan *p) {
    PNPP_REQUIRE(d, PNPP_ERR_ARG, "pt_infer: null descriptor");
    PNPP_REQUIRE(d->B > 0 && d->B <= 65535, PNPP_ERR_ARG, "pt_infer: B=%d outside 1..65535", d->B);
    PNPP_REQUIRE(d->N > 0 && d->N % kPtRows == 0, PNPP_ERR_ARG, "pt_infer: N=%d rows per cloud must be a positive multiple of %d (pad)", d->N,
                 kPtRows);
    PNPP_REQUIRE(d->n_valid > 0 && d->n_valid <= d->N, PNPP_ERR_ARG, "pt_infer: n_valid=%d outside 1..N=%d", d->n_valid, d->N);
    PNPP_REQUIRE(d->in_dim > 0 && d->in_dim <= kPtMaxIn, PNPP_ERR_ARG, "pt_infer: in_dim=%d outside 1..%d", d->in_dim, kPtMaxIn);
    PNPP_REQUIRE(d->E == kPtE, PNPP_ERR_ARG, "pt_infer: E=%d, the fused kernels take an embedding of %d", d->E, kPtE);
    PNPP_REQUIRE(d->H == kPtH, PNPP_ERR_ARG, "pt_infer: H=%d, the fused kernels take %d heads (head dimension 16)", d->H, kPtH);
    PNPP_REQUIRE(d->F > 0 && d->F % kPtChunk == 0, PNPP_ERR_ARG, "pt_infer: F=%d must be a positive multiple of the hidden chunk %d", d->F,
                 kPtChunk);
    PNPP_REQUIRE(d->depth > 0 && d->depth <= 1024, PNPP_ERR_ARG, "pt_infer: depth=%d outside 1..1024", d->depth);
    PNPP_REQUIRE(d->eps > 0.f, PNPP_ERR_ARG, "pt_infer: eps=%g must be positive", (double)d->eps);
    PNPP_REQUIRE((long long)d->B * d->N * 3 * kPtE < (1ll << 31), PNPP_ERR_ARG, "pt_infer: B*N*3E overflows int32");
    p->M = d->B * d->N;
    p->tiles32 = d->N / 32;
    p->scratch_bytes = align_up((size_t)d->B * p->tiles32 * kPtE * sizeof(float), 256);
    return PNPP_OK;
}

static void pt_matrix_shape(const pnpp_pt_infer_desc *d, int m, int *rows, int *ld) {
    *rows = m == PT_IN_PROJ ? 3 * kPtE : m == PT_LINEAR1 ? d->F : kPtE;
    *ld = m == PT_LINEAR2 ? d->F : kPtE;
}

// One blob per layer (so that no allocation of a caller exceeds a layer's planes): the input_proj weight (E x 8 float32, zero beyond
// in_dim; read from layer 0's blob only) and bias, then the layer's matrices and LayerNorms.  The offsets are the same for every layer.
static size_t pt_blob(const pnpp_pt_infer_desc *d, PtLayerOff *o, size_t *wp, size_t *bp) {
    size_t off = 0;
    if (wp) *wp = off;
    off = align_up(off + (size_t)kPtE * kPtMaxIn * sizeof(float), 256);
    if (bp) *bp = off;
    off = align_up(off + (size_t)kPtE * sizeof(float), 256);
    PtLayerOff t;
    for (int m = 0; m < 4; ++m) {
        int rows, ld;
        pt_matrix_shape(d, m, &rows, &ld);
        t.w[m] = off;
        off = align_up(off + (size_t)rows * ld * 3 * sizeof(unsigned short), 256);
        t.b[m] = off;
        off = align_up(off + (size_t)rows * sizeof(float), 256);
    }
    for (int n = 0; n < 2; ++n) {
        t.g[n] = off;
        off = align_up(off + (size_t)kPtE * sizeof(float), 256);
        t.be[n] = off;
        off = align_up(off + (size_t)kPtE * sizeof(float), 256);
    }
    if (o) *o = t;
    return off;
}

// W (C x ld row-major float32) -> the three fragment-major bf16 planes of its exact split (the layout pnpp_sa_infer documents)
__global__ __launch_bounds__(256) void pt_split_weight_kernel(const float *__restrict__ w, int ld, unsigned short *__restrict__ out) {
    const int n = blockIdx.x;
    const size_t plane = (size_t)gridDim.x * ld;
    for (int k = threadIdx.x; k < ld; k += blockDim.x) {
        unsigned h, m, l;
        sp_split2(w[(size_t)n * ld + k], 0.f, h, m, l);
        const size_t at = ((((size_t)(n >> 5) * (ld >> 4) + (k >> 4)) * 64 + (((k & 15) >> 3) << 5) + (n & 31)) << 3) + (k & 7);
        out[at] = (unsigned short)h, out[plane + at] = (unsigned short)m, out[2 * plane + at] = (unsigned short)l;
    }
}

// dst (rows x ldd) = src (rows x lds), zero beyond lds
__global__ __launch_bounds__(256) void pt_copy_pad_kernel(const float *__restrict__ src, int rows, int lds_, int ldd, float *__restrict__ dst) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * ldd) return;
    const int r = e / ldd, c = e % ldd;
    dst[e] = c < lds_ ? src[(size_t)r * lds_ + c] : 0.f;
}

// ---- device routines ------------------------------------------------------------------------------------------------------------
// A wave's 32 x 64 tile in the accumulator layout of v_mfma_f32_32x32x16: v[j][i] is row (i & 3) + 8 (i >> 2) + 4 h, column 32 j + r
// of lane 32 h + r.
__device__ __forceinline__ int pt_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// what a wave wrote to its LDS tile becomes visible to its other lanes (LDS operations of a wave execute in order; this keeps the
// compiler from moving them across)
__device__ __forceinline__ void pt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the tile, split once into its three bf16 planes, as the next product's A operand
__device__ __forceinline__ void pt_store_split(const float (&v)[2][16], unsigned short *__restrict__ tile) {
    const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; i += 2) {   // registers i and i + 1 are rows `row` and `row + 1`
            unsigned ph, pm, pl;
            sp_split2(v[j][i], v[j][i + 1], ph, pm, pl);
            unsigned short *o = tile + pt_row(i, h) * kPtLd + 32 * j + r;
            o[0] = (unsigned short)ph, o[kPtLd] = (unsigned short)(ph >> 16);
            o[kPtPlane] = (unsigned short)pm, o[kPtPlane + kPtLd] = (unsigned short)(pm >> 16);
            o[2 * kPtPlane] = (unsigned short)pl, o[2 * kPtPlane + kPtLd] = (unsigned short)(pl >> 16);
        }
}

__device__ __forceinline__ float pt_sum32(float s) {
#pragma unroll
    for (int m = 1; m <= 16; m <<= 1) s += __shfl_xor(s, m, 64);
    return s;
}

// v = LayerNorm(v) over the 64 columns of each row: two passes, as add_layernorm_kernel
__device__ __forceinline__ void pt_layernorm(float (&v)[2][16], const float *__restrict__ gamma, const float *__restrict__ beta, float eps) {
    const int r = threadIdx.x & 31;
    const float g0 = gamma[r], g1 = gamma[32 + r], b0 = beta[r], b1 = beta[32 + r];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float mu = pt_sum32(v[0][i] + v[1][i]) * (1.f / kPtE);
        const float d0 = v[0][i] - mu, d1 = v[1][i] - mu;
        const float var = pt_sum32(d0 * d0 + d1 * d1) * (1.f / kPtE);
        const float is = 1.f / sqrtf(var + eps);
        v[0][i] = d0 * is * g0 + b0;
        v[1][i] = d1 * is * g1 + b1;
    }
}

// acc = tile (32 x 64) * W[col0 .. col0 + 64)[0 .. 64)^T, W in fragment-major planes `wplane` apart
__device__ __forceinline__ void pt_product(const unsigned short *__restrict__ tile, const unsigned short *__restrict__ W, size_t wplane, int col0,
                                           f32x16 (&acc)[2]) {
    f32x16 accl[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f, accl[j][i] = 0.f;
    infer_chunk<2>(tile, kPtLd, (size_t)kPtPlane, kPtE, W, wplane, col0, 32, acc, accl);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] += accl[j][i];
}

// qkv[row0 .. row0 + 32) = tile W_in^T + b_in (3E = 192 columns)
__device__ __forceinline__ void pt_in_proj(const unsigned short *__restrict__ tile, const unsigned short *__restrict__ w_in,
                                           const float *__restrict__ b_in, float *__restrict__ qkv, size_t row0) {
    const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
    for (int c0 = 0; c0 < 3 * kPtE; c0 += 64) {
        f32x16 acc[2];
        pt_product(tile, w_in, (size_t)3 * kPtE * kPtE, c0, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = c0 + 32 * j + r;
            const float bc = b_in[col];
#pragma unroll
            for (int i = 0; i < 16; ++i) qkv[(row0 + pt_row(i, h)) * (3 * kPtE) + col] = acc[j][i] + bc;
        }
    }
}

struct PtHeadArgs {
    const float *xyz;            // (B, n_valid, in_dim)
    const float *wp, *bp;        // (E, 8), (E)
    const unsigned short *w_in;  // layer 0's in_proj planes
    const float *b_in;
    float *x0, *qkv0;
    const int *lengths;          // (B) int32 or null: the ragged form, cloud b holds min(max(lengths[b], 1), n_valid) points
    int N, n_valid, in_dim;
};

// the points of cloud b: n_valid, or in the ragged form the cloud's own length, clamped into 1 .. n_valid
__device__ __forceinline__ int pt_cloud_rows(const int *__restrict__ lengths, int b, int n_valid) {
    return lengths ? min(max(lengths[b], 1), n_valid) : n_valid;
}

__global__ __launch_bounds__(kPtThreads) void pt_head_infer_kernel(const PtHeadArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
    unsigned short *tile = lds + wave * kPtTile;
    const size_t row0 = (size_t)blockIdx.x * kPtRows + wave * 32;
    const int b = (int)(row0 / P.N), n0 = (int)(row0 % P.N);
    const int len = pt_cloud_rows(P.lengths, b, P.n_valid);   // every row is written on every call, whatever the length: the next kernels read them
    float w[2][kPtMaxIn], bias[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        bias[j] = P.bp[32 * j + r];
#pragma unroll
        for (int k = 0; k < kPtMaxIn; ++k) w[j][k] = P.wp[(32 * j + r) * kPtMaxIn + k];   // zero beyond in_dim
    }
    float v[2][16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = n0 + pt_row(i, h);
        const float *xr = P.xyz + ((size_t)b * P.n_valid + n) * P.in_dim;
        float a0 = bias[0], a1 = bias[1];
#pragma unroll
        for (int k = 0; k < kPtMaxIn; ++k) {
            const float x = (n < len && k < P.in_dim) ? xr[k] : 0.f;   // rows beyond the cloud are zero points, whatever they hold
            a0 = fmaf(x, w[0][k], a0), a1 = fmaf(x, w[1][k], a1);
        }
        v[0][i] = a0, v[1][i] = a1;
        float *xo = P.x0 + (row0 + pt_row(i, h)) * kPtE;
        xo[r] = a0, xo[32 + r] = a1;
    }
    pt_store_split(v, tile);
    pt_wave_sync();
    pt_in_proj(tile, P.w_in, P.b_in, P.qkv0, row0);
}

struct PtTailArgs {
    const float *x, *o;                        // (M, E): the layer's input, the attention output
    const unsigned short *w_out, *w1, *w2;     // planes of out_proj (E x E), linear1 (F x E), linear2 (E x F)
    const float *b_out, *b1, *b2;
    const float *g1, *be1, *g2, *be2;          // norm1, norm2
    const unsigned short *w_in;                // the next layer's in_proj planes, or null in the last layer
    const float *b_in;
    float *x_next, *qkv_next, *part;           // (M, E); (M, 3E) or null; (B, N/32, E) or null
    const int *lengths;                        // (B) int32 or null, as PtHeadArgs: only the last layer's pooling looks at it
    int N, n_valid, F;
    float eps;
};

// the 48 KiB of chunk c: thread t takes uint4 number 256 i + t of the W_1 part (i < 6) and of the W_2 part
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void pt_fetch_chunk(const PtTailArgs &P, int c, u32x4 (&pf)[12]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        // W_1: plane i / 2; the chunk's two column blocks are 4096 consecutive elements of a plane
        pf[i] = *reinterpret_cast<const u32x4 *>(P.w1 + (size_t)(i >> 1) * P.F * kPtE + (size_t)c * kPtWPlane + ((i & 1) * 256 + t) * 8);
        // W_2: plane i / 2, column block i & 1; the chunk's four reduction steps are 2048 consecutive elements of a column block
        pf[6 + i] = *reinterpret_cast<const u32x4 *>(P.w2 + (size_t)(i >> 1) * kPtE * P.F + ((size_t)(i & 1) * (P.F >> 4) + 4 * c) * 512 + t * 8);
    }
}

__global__ __launch_bounds__(kPtThreads) void pt_tail_infer_kernel(const PtTailArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
    unsigned short *wbuf = lds;                                       // W_1 chunk planes, then W_2 chunk planes
    unsigned short *ut = lds + kPtWChunk + wave * kPtTile;            // u, later y: the wave's rows
    unsigned short *ht = lds + kPtWChunk + (4 + wave) * kPtTile;      // the attention output, then the hidden chunks
    const size_t row0 = (size_t)blockIdx.x * kPtRows + wave * 32;
    u32x4 pf[12];
    pt_fetch_chunk(P, 0, pf);

    // 1. u = LN1(x + o W_out^T + b_out)
    float v[2][16];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) v[j][i] = P.o[(row0 + pt_row(i, h)) * kPtE + 32 * j + r];
    pt_store_split(v, ht);
    pt_wave_sync();
    {
        f32x16 acc[2];
        pt_product(ht, P.w_out, (size_t)kPtE * kPtE, 0, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float bc = P.b_out[32 * j + r];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[j][i] = P.x[(row0 + pt_row(i, h)) * kPtE + 32 * j + r] + (acc[j][i] + bc);
        }
    }
    pt_layernorm(v, P.g1, P.be1, P.eps);
    pt_store_split(v, ut);
    pt_wave_sync();

    // 2. y = u + relu(u W_1^T + b_1) W_2^T + b_2, 64 hidden columns at a time
    f32x16 y[2], yl[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) y[j][i] = 0.f, yl[j][i] = 0.f;
    const int nchunk = P.F / kPtChunk;
    for (int c = 0; c < nchunk; ++c) {
        __syncthreads();   // every wave is done with the previous chunk's weights
#pragma unroll
        for (int i = 0; i < 12; ++i) reinterpret_cast<u32x4 *>(wbuf)[(i < 6 ? 0 : 1536) + (i % 6) * 256 + threadIdx.x] = pf[i];
        __syncthreads();
        pt_fetch_chunk(P, c + 1 < nchunk ? c + 1 : c, pf);   // in flight while this chunk is multiplied (the last one fetches itself again)
        f32x16 acc[2];
        pt_product(ut, wbuf, (size_t)kPtWPlane, 0, acc);
        float t[2][16];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float bc = P.b1[c * kPtChunk + 32 * j + r];
#pragma unroll
            for (int i = 0; i < 16; ++i) t[j][i] = fmaxf(acc[j][i] + bc, 0.f);
        }
        pt_store_split(t, ht);
        pt_wave_sync();
        infer_chunk<2>(ht, kPtLd, (size_t)kPtPlane, kPtChunk, wbuf + 3 * kPtWPlane, (size_t)kPtWPlane, 0, 32, y, yl);
    }

    // 3. x_next = LN2(u + y + b_2)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float bc = P.b2[32 * j + r];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[j][i] += (y[j][i] + yl[j][i]) + bc;
    }
    pt_layernorm(v, P.g2, P.be2, P.eps);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) P.x_next[(row0 + pt_row(i, h)) * kPtE + 32 * j + r] = v[j][i];

    // 4. the next layer's in_proj, or the pooled sums over the block's valid rows
    if (P.w_in) {
        pt_store_split(v, ut);
        pt_wave_sync();
        pt_in_proj(ut, P.w_in, P.b_in, P.qkv_next, row0);
    } else {
        const int b = (int)(row0 / P.N), n0 = (int)(row0 % P.N);
        const int len = pt_cloud_rows(P.lengths, b, P.n_valid);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) s += (n0 + pt_row(i, h) < len) ? v[j][i] : 0.f;   // padding rows are never pooled
            s += __shfl_xor(s, 32, 64);
            if (h == 0) P.part[((size_t)b * (P.N / 32) + n0 / 32) * kPtE + 32 * j + r] = s;
        }
    }
}

// out[b] = (sum of the cloud's partial rows / n_valid) W_fc^T + b_fc; one wave per cloud, float64, fixed order
__global__ __launch_bounds__(64) void pt_pool_infer_kernel(const float *__restrict__ part, int tiles, int n_valid, const int *__restrict__ lengths,
                                                           const float *__restrict__ fw, const float *__restrict__ fb, int n_out,
                                                           float *__restrict__ out) {
    __shared__ double mean[kPtE];
    const int b = blockIdx.x, c = threadIdx.x;
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += (double)part[((size_t)b * tiles + t) * kPtE + c];   // blocks beyond the cloud hold exact zeros
    mean[c] = s / (double)pt_cloud_rows(lengths, b, n_valid);
    __syncthreads();
    for (int o = c; o < n_out; o += 64) {
        double a = (double)fb[o];
        for (int k = 0; k < kPtE; ++k) a += mean[k] * (double)fw[(size_t)o * kPtE + k];
        out[(size_t)b * n_out + o] = (float)a;
    }
}

// dynamic LDS above 48 KiB has to be allowed once per kernel (process-wide flag: one process drives one GPU)
static int pt_allow_lds(const void *fn, size_t bytes, bool *granted, const char *what) {
    if (*granted) return PNPP_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    PNPP_REQUIRE(e == hipSuccess, PNPP_ERR_LAUNCH, "%s: cannot allow %zu bytes of dynamic LDS: %s", what, bytes, hipGetErrorString(e));
    *granted = true;
    return PNPP_OK;
}

}  // namespace
}  // namespace pnpp

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace pnpp;

extern "C" int pnpp_pt_infer_supported(const pnpp_pt_infer_desc *d) {
    PtPlan p;
    return pt_plan(d, &p) == PNPP_OK ? 1 : 0;
}

extern "C" size_t pnpp_pt_infer_weights_bytes(const pnpp_pt_infer_desc *d) {
    PtPlan p;
    if (pt_plan(d, &p) != PNPP_OK) return 0;
    return pt_blob(d, nullptr, nullptr, nullptr);
}

extern "C" size_t pnpp_pt_infer_scratch_bytes(const pnpp_pt_infer_desc *d) {
    PtPlan p;
    if (pt_plan(d, &p) != PNPP_OK) return 0;
    return p.scratch_bytes;
}

extern "C" int pnpp_pt_infer_weights_layout(const pnpp_pt_infer_desc *d, int layer, int matrix, size_t *w_offset_host, int *w_ld_host,
                                            size_t *b_offset_host) {
    PtPlan p;
    int rc = pt_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(w_offset_host && w_ld_host && b_offset_host, PNPP_ERR_ARG, "pt_infer_weights_layout: null pointer");
    PNPP_REQUIRE(matrix >= PT_IN_PROJ && matrix <= PT_INPUT_PROJ, PNPP_ERR_ARG, "pt_infer_weights_layout: matrix %d outside 0..6", matrix);
    PNPP_REQUIRE(layer >= 0 && layer < d->depth, PNPP_ERR_ARG, "pt_infer_weights_layout: layer %d outside 0..%d", layer, d->depth - 1);
    PtLayerOff o;
    size_t wp, bp;
    pt_blob(d, &o, &wp, &bp);
    if (matrix == PT_INPUT_PROJ) {
        *w_offset_host = wp, *b_offset_host = bp, *w_ld_host = kPtMaxIn;
    } else if (matrix <= PT_LINEAR2) {
        int rows;
        pt_matrix_shape(d, matrix, &rows, w_ld_host);
        *w_offset_host = o.w[matrix], *b_offset_host = o.b[matrix];
    } else {
        *w_offset_host = o.g[matrix - PT_NORM1], *b_offset_host = o.be[matrix - PT_NORM1], *w_ld_host = kPtE;
    }
    return PNPP_OK;
}

extern "C" int pnpp_pt_infer_fold(const pnpp_pt_infer_desc *d, int layer, const pnpp_pt_infer_layer_params *q, const float *input_w,
                                  const float *input_b, void *weights, void *stream) {
    PtPlan p;
    int rc = pt_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(layer >= 0 && layer < d->depth, PNPP_ERR_ARG, "pt_infer_fold: layer %d outside 0..%d", layer, d->depth - 1);
    PNPP_REQUIRE(q && weights, PNPP_ERR_ARG, "pt_infer_fold: null pointer");
    PNPP_REQUIRE(layer > 0 || (input_w && input_b), PNPP_ERR_ARG, "pt_infer_fold: layer 0 needs input_proj, got a null pointer");
    PNPP_REQUIRE(q->in_proj_w && q->in_proj_b && q->out_proj_w && q->out_proj_b && q->linear1_w && q->linear1_b && q->linear2_w && q->linear2_b &&
                     q->norm1_w && q->norm1_b && q->norm2_w && q->norm2_b,
                 PNPP_ERR_ARG, "pt_infer_fold: null parameter pointer in layer %d", layer);
    hipStream_t st = as_stream(stream);
    char *base = static_cast<char *>(weights);
    auto copy = [&](const float *src, int rows, int lds_, int ldd, size_t off) {
        ProfScope ps(st, "pt_copy_pad_kernel rows=%d ld=%d", rows, ldd);
        hipLaunchKernelGGL(pt_copy_pad_kernel, dim3(cdiv(rows * ldd, 256)), dim3(256), 0, st, src, rows, lds_, ldd,
                           reinterpret_cast<float *>(base + off));
    };
    size_t wp, bp;
    PtLayerOff o;
    pt_blob(d, &o, &wp, &bp);
    if (layer == 0) {
        copy(input_w, kPtE, d->in_dim, kPtMaxIn, wp);
        copy(input_b, 1, kPtE, kPtE, bp);
    }
    const float *w[4] = {q->in_proj_w, q->out_proj_w, q->linear1_w, q->linear2_w};
    const float *b[4] = {q->in_proj_b, q->out_proj_b, q->linear1_b, q->linear2_b};
    for (int m = 0; m < 4; ++m) {
        int rows, ld;
        pt_matrix_shape(d, m, &rows, &ld);
        {
            ProfScope ps(st, "pt_split_weight_kernel C=%d ld=%d", rows, ld);
            hipLaunchKernelGGL(pt_split_weight_kernel, dim3(rows), dim3(256), 0, st, w[m], ld, reinterpret_cast<unsigned short *>(base + o.w[m]));
        }
        copy(b[m], 1, rows, rows, o.b[m]);
    }
    copy(q->norm1_w, 1, kPtE, kPtE, o.g[0]), copy(q->norm1_b, 1, kPtE, kPtE, o.be[0]);
    copy(q->norm2_w, 1, kPtE, kPtE, o.g[1]), copy(q->norm2_b, 1, kPtE, kPtE, o.be[1]);
    PNPP_CHECK_LAUNCH("pt_infer_fold");
    return PNPP_OK;
}

// lengths == nullptr: the uniform call; otherwise the ragged one (the _ragged entry points refuse a null tensor before they come here)
static int pt_infer_head_launch(const pnpp_pt_infer_desc *d, const int32_t *lengths, const float *xyz, const void *weights0, float *x0, float *qkv0,
                                void *stream) {
    PtPlan p;
    int rc = pt_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(xyz && weights0 && x0 && qkv0, PNPP_ERR_ARG, "pt_infer_head: null pointer");
    const char *base = static_cast<const char *>(weights0);
    size_t wp, bp;
    PtLayerOff o;
    pt_blob(d, &o, &wp, &bp);
    PtHeadArgs P;
    P.xyz = xyz, P.wp = reinterpret_cast<const float *>(base + wp), P.bp = reinterpret_cast<const float *>(base + bp);
    P.w_in = reinterpret_cast<const unsigned short *>(base + o.w[PT_IN_PROJ]), P.b_in = reinterpret_cast<const float *>(base + o.b[PT_IN_PROJ]);
    P.x0 = x0, P.qkv0 = qkv0, P.lengths = lengths, P.N = d->N, P.n_valid = d->n_valid, P.in_dim = d->in_dim;
    static bool granted = false;
    rc = pt_allow_lds((const void *)pt_head_infer_kernel, kPtHeadLds, &granted, "pt_infer_head");
    if (rc != PNPP_OK) return rc;
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, lengths ? "pt_head_infer_kernel M=%d E=%d F=%d K=%d valid=%d ragged=1" : "pt_head_infer_kernel M=%d E=%d F=%d K=%d valid=%d", p.M, kPtE,
                 d->F, d->in_dim, d->n_valid);
    hipLaunchKernelGGL(pt_head_infer_kernel, dim3(p.M / kPtRows), dim3(kPtThreads), kPtHeadLds, st, P);
    PNPP_CHECK_LAUNCH("pt_infer_head");
    return PNPP_OK;
}

extern "C" int pnpp_pt_infer_head(const pnpp_pt_infer_desc *d, const float *xyz, const void *weights0, float *x0, float *qkv0, void *stream) {
    return pt_infer_head_launch(d, nullptr, xyz, weights0, x0, qkv0, stream);
}

extern "C" int pnpp_pt_infer_head_ragged(const pnpp_pt_infer_desc *d, const int32_t *lengths, const float *xyz, const void *weights0, float *x0,
                                         float *qkv0, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "pt_infer_head_ragged: null lengths pointer (the uniform call is pnpp_pt_infer_head)");
    return pt_infer_head_launch(d, lengths, xyz, weights0, x0, qkv0, stream);
}

static int pt_infer_tail_launch(const pnpp_pt_infer_desc *d, const int32_t *lengths, int layer, const float *x, const float *o, const void *weights,
                                const void *weights_next, float *x_next, float *qkv_next, void *scratch, void *stream) {
    PtPlan p;
    int rc = pt_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(layer >= 0 && layer < d->depth, PNPP_ERR_ARG, "pt_infer_tail: layer %d outside 0..%d", layer, d->depth - 1);
    const bool last = layer == d->depth - 1;
    PNPP_REQUIRE(x && o && weights && x_next, PNPP_ERR_ARG, "pt_infer_tail: null pointer");
    PNPP_REQUIRE(last ? scratch != nullptr : (qkv_next != nullptr && weights_next != nullptr), PNPP_ERR_ARG,
                 "pt_infer_tail: null %s pointer in layer %d", last ? "scratch" : "qkv_next / weights_next", layer);
    PNPP_REQUIRE(x_next != x && x_next != o, PNPP_ERR_ARG, "pt_infer_tail: x_next must not alias x or o");
    const char *base = static_cast<const char *>(weights);
    PtLayerOff w;
    pt_blob(d, &w, nullptr, nullptr);
    auto planes = [&](const char *bs, size_t off) { return reinterpret_cast<const unsigned short *>(bs + off); };
    auto floats = [&](const char *bs, size_t off) { return reinterpret_cast<const float *>(bs + off); };
    PtTailArgs P;
    P.x = x, P.o = o;
    P.w_out = planes(base, w.w[PT_OUT_PROJ]), P.w1 = planes(base, w.w[PT_LINEAR1]), P.w2 = planes(base, w.w[PT_LINEAR2]);
    P.b_out = floats(base, w.b[PT_OUT_PROJ]), P.b1 = floats(base, w.b[PT_LINEAR1]), P.b2 = floats(base, w.b[PT_LINEAR2]);
    P.g1 = floats(base, w.g[0]), P.be1 = floats(base, w.be[0]), P.g2 = floats(base, w.g[1]), P.be2 = floats(base, w.be[1]);
    P.w_in = nullptr, P.b_in = nullptr, P.qkv_next = nullptr, P.part = nullptr;
    if (last) {
        P.part = static_cast<float *>(scratch);
    } else {
        const char *nb = static_cast<const char *>(weights_next);
        P.w_in = planes(nb, w.w[PT_IN_PROJ]), P.b_in = floats(nb, w.b[PT_IN_PROJ]), P.qkv_next = qkv_next;
    }
    P.x_next = x_next, P.lengths = lengths, P.N = d->N, P.n_valid = d->n_valid, P.F = d->F, P.eps = d->eps;
    static bool granted = false;
    rc = pt_allow_lds((const void *)pt_tail_infer_kernel, kPtTailLds, &granted, "pt_infer_tail");
    if (rc != PNPP_OK) return rc;
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, lengths ? "pt_tail_infer_kernel M=%d E=%d F=%d valid=%d last=%d ragged=1" : "pt_tail_infer_kernel M=%d E=%d F=%d valid=%d last=%d", p.M, kPtE,
                 d->F, d->n_valid, last ? 1 : 0);
    hipLaunchKernelGGL(pt_tail_infer_kernel, dim3(p.M / kPtRows), dim3(kPtThreads), kPtTailLds, st, P);
    PNPP_CHECK_LAUNCH("pt_infer_tail");
    return PNPP_OK;
}

extern "C" int pnpp_pt_infer_tail(const pnpp_pt_infer_desc *d, int layer, const float *x, const float *o, const void *weights,
                                  const void *weights_next, float *x_next, float *qkv_next, void *scratch, void *stream) {
    return pt_infer_tail_launch(d, nullptr, layer, x, o, weights, weights_next, x_next, qkv_next, scratch, stream);
}

extern "C" int pnpp_pt_infer_tail_ragged(const pnpp_pt_infer_desc *d, const int32_t *lengths, int layer, const float *x, const float *o,
                                         const void *weights, const void *weights_next, float *x_next, float *qkv_next, void *scratch,
                                         void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "pt_infer_tail_ragged: null lengths pointer (the uniform call is pnpp_pt_infer_tail)");
    return pt_infer_tail_launch(d, lengths, layer, x, o, weights, weights_next, x_next, qkv_next, scratch, stream);
}

static int pt_infer_pool_launch(const pnpp_pt_infer_desc *d, const int32_t *lengths, const void *scratch, const float *fc_w, const float *fc_b,
                                int n_out, float *out, void *stream) {
    PtPlan p;
    int rc = pt_plan(d, &p);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(scratch && fc_w && fc_b && out, PNPP_ERR_ARG, "pt_infer_pool: null pointer");
    PNPP_REQUIRE(n_out > 0, PNPP_ERR_ARG, "pt_infer_pool: n_out=%d must be positive", n_out);
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, lengths ? "pt_pool_infer_kernel M=%d E=%d F=%d B=%d valid=%d out=%d ragged=1" : "pt_pool_infer_kernel M=%d E=%d F=%d B=%d valid=%d out=%d",
                 p.M, kPtE, d->F, d->B, d->n_valid, n_out);
    hipLaunchKernelGGL(pt_pool_infer_kernel, dim3(d->B), dim3(64), 0, st, static_cast<const float *>(scratch), p.tiles32, d->n_valid, lengths, fc_w,
                       fc_b, n_out, out);
    PNPP_CHECK_LAUNCH("pt_infer_pool");
    return PNPP_OK;
}

extern "C" int pnpp_pt_infer_pool(const pnpp_pt_infer_desc *d, const void *scratch, const float *fc_w, const float *fc_b, int n_out, float *out,
                                  void *stream) {
    return pt_infer_pool_launch(d, nullptr, scratch, fc_w, fc_b, n_out, out, stream);
}

extern "C" int pnpp_pt_infer_pool_ragged(const pnpp_pt_infer_desc *d, const int32_t *lengths, const void *scratch, const float *fc_w,
                                         const float *fc_b, int n_out, float *out, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "pt_infer_pool_ragged: null lengths pointer (the uniform call is pnpp_pt_infer_pool)");
    return pt_infer_pool_launch(d, lengths, scratch, fc_w, fc_b, n_out, out, stream);
}
