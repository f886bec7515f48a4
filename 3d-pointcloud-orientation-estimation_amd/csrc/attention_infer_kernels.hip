// attention_infer_kernels.hip -- forward-only attention of the point transformer's Predictor (pnpp_attention_infer): what
// attention_fwd_kernel (transformer_kernels.hip) computes with lse = NULL and mask = NULL, with both products on
// v_mfma_f32_32x32x16_bf16 from the exact three-way bf16 splits of their float32 operands (split_infer.h) in place of
// v_mfma_f32_32x32x2_f32.  Same buffers, same padding contract: N a multiple of 128, keys >= n_valid get no weight, key blocks without a
// point are not visited, padded query rows are computed like any other (finite for finite input).
// Ragged form (pnpp_attention_infer_ragged, `lengths` non-null): n_valid becomes the cloud's own min(max(lengths[b], 1), n_valid), rows
// from there on are written as zeros, and a workgroup wholly beyond its cloud writes its zeros and leaves before any barrier.
//
// Workgroup = 128 queries of one (cloud, head): 4 waves x 32 queries, as the float32 kernel.  Keys / values stream through LDS in
// stages of 64 (two 32-key tiles), double buffered, one barrier per stage; they are split into their three planes while they are
// staged, once per workgroup, and the query rows once per lane.
//
// Layouts (v_mfma_f32_32x32x16_bf16: lane 32 h + r holds A[row r][k = 8 h + j] and B[k = 8 h + j][column r], j = 0 .. 7;
// D[row (r & 3) + 8 (r >> 2) + 4 h][column = lane & 31] in register r):
//   S^T = K Q^T : A = key tile (row = key, k = dim), B = Q^T (k = dim, column = query): head dimension 16 is one instruction per partial
//                 product.  A lane is a query and register r holds key kappa(r, h) = (r & 3) + 8 (r >> 2) + 4 h, as in the float32
//                 kernel.  K planes in LDS: [dims 0..7 | dims 8..15][key][8], so a lane's fragment is one 16-byte read.
//   O^T = V^T P^T: the k index of a step may name any key as long as A and B agree.  Step u takes this lane's probability registers
//                 8 u .. 8 u + 7 as its B fragment, k = 8 h + j naming key kappa(8 u + j, h) = 16 u + 4 h + j (j < 4) and
//                 16 u + 8 + 4 h + (j - 4): the probabilities never move between lanes.  The A fragment is then two runs of four keys
//                 of one dim; the V^T planes in LDS are key-contiguous with the keys of a group of 16 stored in the order
//                 4 h + j, 8 + 4 h + j, so the two runs are adjacent and a fragment is again one 16-byte read.
//   Rows 16 .. 31 of V^T do not exist at head dimension 16.  Row 16 of the leading plane holds ones (exact in bf16), the rest zeros,
//   written once: row 16 of O^T is then the sum of the probabilities, rescaled with the rest, and no row sum is formed on the VALU.
//
// Products kept: all six of split_infer.h in both products, the leading one in its own accumulator (infer_chunk's comment says why);
// the three dropped terms together lie below 2^-26 |a| |b|.  DESIGN section 11 has the bound, the instruction counts and the measurements.
#include "common.h"
#include "split_infer.h"

// No contraction of a * b + c into a fused multiply-add the source does not spell: the rescale needs ml = m * log2(e) ROUNDED, so that a
// row whose maximum did not move gets alpha = exp2(ml - ml) = 1 exactly (the rescale branch is wave-uniform: such rows pass through it
// whenever another row of the wave moved, and must come out bit for bit as if they had not).  The one fma wanted is written fmaf.
#pragma clang fp contract(off)

namespace pnpp {
namespace {

constexpr int AI_DH = 16;                  // head dimension
constexpr int AI_KS = 64;                  // keys per stage
constexpr int AI_KPLANE = 2 * AI_KS * 8;   // bf16 per K plane: [2 dim halves][64 keys][8 dims]
constexpr int AI_VP = AI_KS + 8;           // pitch of a V^T row in bf16: 144 bytes, 16-byte reads of 32 consecutive rows hit every bank once
constexpr int AI_VPLANE = 32 * AI_VP;      // bf16 per V^T plane: 16 dims + the ones row + 15 zero rows
constexpr float AI_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ f32x16 ai_mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

__global__ void __launch_bounds__(256, 4)   // at least four waves per SIMD (here: four workgroups per CU): a wave's softmax and splits issue beside the MFMAs of three others
attention_infer_kernel(const float *__restrict__ qkv, int N, int Nv, const int *__restrict__ lengths, int H, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned short Ks[2][3][AI_KPLANE];
    __shared__ __attribute__((aligned(16))) unsigned short Vs[2][3][AI_VPLANE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z, E = H * AI_DH, ld = 3 * E;
    const float *base = qkv + (size_t)b * N * ld;
    const int q = blockIdx.x * 128 + wave * 32 + l31;   // this lane's query (N % 128 == 0: the row exists)
    const int Nz = att_ragged_rows(lengths, b, N, Nv);  // ragged form: Nv becomes the cloud's own length, rows from Nz on are written as zeros
    if ((int)blockIdx.x * 128 >= Nz) {                  // a workgroup wholly beyond its cloud (by blockIdx: all of it leaves before any barrier)
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 *orow = reinterpret_cast<float4 *>(out + ((size_t)b * N + q) * E + h * AI_DH + 4 * lh);
        orow[0] = z, orow[2] = z;
        return;
    }

    // rows 16 .. 31 of the V^T planes, both buffers: ones in row 16 of the leading plane, zeros elsewhere; staging never writes them
    for (int i = tid; i < 2 * 3 * 8 * AI_VP; i += 256) {   // 32-bit words
        const int bp = i / (8 * AI_VP), e = i % (8 * AI_VP);
        reinterpret_cast<unsigned *>(&Vs[0][0][0])[bp * (AI_VPLANE / 2) + 8 * AI_VP + e] = (bp % 3 == 0 && e < AI_VP / 2) ? 0x3F803F80u : 0u;
    }

    // Q^T operand: dims 8 h .. 8 h + 7 of this lane's query, scaled by 1 / sqrt(16) (a power of two: the split stays exact)
    bf16x8 qh, qm, ql;
    {
        const float4 *qp = reinterpret_cast<const float4 *>(base + (size_t)q * ld + h * AI_DH + 8 * lh);
        const float4 a = qp[0], c = qp[1];
        unsigned ph[4], pm[4], pl[4];
        sp_split2(a.x * 0.25f, a.y * 0.25f, ph[0], pm[0], pl[0]);
        sp_split2(a.z * 0.25f, a.w * 0.25f, ph[1], pm[1], pl[1]);
        sp_split2(c.x * 0.25f, c.y * 0.25f, ph[2], pm[2], pl[2]);
        sp_split2(c.z * 0.25f, c.w * 0.25f, ph[3], pm[3], pl[3]);
        qh = sp_frag(ph), qm = sp_frag(pm), ql = sp_frag(pl);
    }

    // staging map.  K: thread = (key, four dims), one float4.  V: thread = (dim, four consecutive keys), so that the split leaves a
    // run of four keys of one dim per plane: one 8-byte write into the key-contiguous image.
    const int k_key = tid >> 2, k_c4 = 4 * (tid & 3);
    const float *k_src = base + E + h * AI_DH + k_c4 + (size_t)k_key * ld;
    const int k_dst = (k_c4 >> 3) * (AI_KS * 8) + k_key * 8 + (k_c4 & 7);
    const int v_dim = tid & 15, v_kg = tid >> 4;
    const float *v_src = base + 2 * E + h * AI_DH + v_dim + (size_t)(4 * v_kg) * ld;
    const int v_dst = v_dim * AI_VP + 16 * (v_kg >> 2) + 8 * (v_kg & 1) + 4 * ((v_kg >> 1) & 1);
    float4 kf;
    float vf[4];
    auto fetch = [&](int st) {   // rows st * 64 .. + 63 exist: the stages cover ceil(Nv / 64) * 64 <= N rows
        const size_t row = (size_t)st * AI_KS * ld;
        kf = *reinterpret_cast<const float4 *>(k_src + row);
#pragma unroll
        for (int i = 0; i < 4; ++i) vf[i] = v_src[row + (size_t)i * ld];
    };
    auto put = [&](int buf) {
        unsigned a[3], c[3];
        sp_split2(kf.x, kf.y, a[0], a[1], a[2]);
        sp_split2(kf.z, kf.w, c[0], c[1], c[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2 *>(&Ks[buf][p][k_dst]) = make_uint2(a[p], c[p]);
        sp_split2(vf[0], vf[1], a[0], a[1], a[2]);
        sp_split2(vf[2], vf[3], c[0], c[1], c[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2 *>(&Vs[buf][p][v_dst]) = make_uint2(a[p], c[p]);
    };

    f32x16 o, ol, zero;   // O^T: the leading products and the five small ones; row 16 (register 8 of the lower half-wave) = sum of p
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f, ol[r] = 0.f, zero[r] = 0.f;
    float m_run = -INFINITY, ml_run = -INFINITY;   // running row maximum and the same times log2(e), as it is rounded

    const int nst = (Nv + AI_KS - 1) / AI_KS;
    fetch(0);
    put(0);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) fetch(st + 1);   // in flight while this stage is computed
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k0 = st * AI_KS + 32 * t;
            if (k0 >= Nv) break;   // a key block without a point
            f32x16 s, sl;
            {
                const unsigned short *kp = &Ks[buf][0][lh * (AI_KS * 8) + (32 * t + l31) * 8];
                const bf16x8 kh = *reinterpret_cast<const bf16x8 *>(kp), km = *reinterpret_cast<const bf16x8 *>(kp + AI_KPLANE),
                             kl = *reinterpret_cast<const bf16x8 *>(kp + 2 * AI_KPLANE);
                s = ai_mfma(kh, qh, zero);
                sl = ai_mfma(kl, qh, zero);
                sl = ai_mfma(kh, ql, sl);
                sl = ai_mfma(km, qm, sl);
                sl = ai_mfma(km, qh, sl);
                sl = ai_mfma(kh, qm, sl);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] += sl[r];
            if (k0 + 32 > Nv) {   // the last block of a cloud whose size is not a multiple of 32
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = k0 + (r & 3) + 8 * (r >> 2) + 4 * lh < Nv ? s[r] : -INFINITY;
            }
            float mx = s[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (__builtin_amdgcn_ballot_w64(mx > m_run) != 0ull) {   // wave-uniform: no row maximum moved, nothing to rescale
                const float m_new = fmaxf(m_run, mx), ml_new = m_new * AI_LOG2E;
                const float alpha = __builtin_amdgcn_exp2f(ml_run - ml_new);   // exp2(-inf) = 0 on the first block
#pragma unroll
                for (int r = 0; r < 9; ++r) o[r] *= alpha, ol[r] *= alpha;
                m_run = m_new, ml_run = ml_new;
            }
            // p = exp(s - m) = exp2(s log2(e) - ml): one fma and one v_exp_f32; the rounding of ml is common to a row's numerator and
            // denominator, and alpha above moves between two rounded values exactly as the probabilities do
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], AI_LOG2E, -ml_run));
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                unsigned ph[4], pm[4], pl[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) sp_split2(s[8 * u + 2 * i], s[8 * u + 2 * i + 1], ph[i], pm[i], pl[i]);
                const bf16x8 bh = sp_frag(ph), bm = sp_frag(pm), bl = sp_frag(pl);
                const unsigned short *vp = &Vs[buf][0][l31 * AI_VP + (2 * t + u) * 16 + lh * 8];
                const bf16x8 vh = *reinterpret_cast<const bf16x8 *>(vp), vm = *reinterpret_cast<const bf16x8 *>(vp + AI_VPLANE),
                             vl = *reinterpret_cast<const bf16x8 *>(vp + 2 * AI_VPLANE);
                o = ai_mfma(vh, bh, o);
                ol = ai_mfma(vl, bh, ol);
                ol = ai_mfma(vh, bl, ol);
                ol = ai_mfma(vm, bm, ol);
                ol = ai_mfma(vm, bh, ol);
                ol = ai_mfma(vh, bm, ol);
            }
        }
        if (st + 1 < nst) put(buf ^ 1);   // the other buffer was last read before the previous barrier
        __syncthreads();
    }
    float t[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) t[r] = o[r] + ol[r];
    const float l = t[8] + __shfl_xor(t[8], 32, 64);   // row 16 sits in the lower half-wave, the upper one holds zero row 20 there
    const float inv = q < Nz ? 1.f / l : 0.f;   // ragged form: a padding query's row is written as zeros (its sums are finite: the keys are points)
    float4 *orow = reinterpret_cast<float4 *>(out + ((size_t)b * N + q) * E + h * AI_DH + 4 * lh);
    orow[0] = make_float4(t[0] * inv, t[1] * inv, t[2] * inv, t[3] * inv);   // dims 4 h + 0 .. 3
    orow[2] = make_float4(t[4] * inv, t[5] * inv, t[6] * inv, t[7] * inv);   // dims 8 + 4 h + 0 .. 3
}

int ai_check(const char *who, int B, int N, int n_valid, int H, int head_dim) {
    PNPP_REQUIRE(B >= 1, PNPP_ERR_ARG, "%s: B=%d, at least one cloud is needed", who, B);
    PNPP_REQUIRE(H >= 1, PNPP_ERR_ARG, "%s: H=%d, at least one head is needed", who, H);
    PNPP_REQUIRE(head_dim == AI_DH, PNPP_ERR_ARG, "%s: head_dim=%d is not supported (only %d)", who, head_dim, AI_DH);
    PNPP_REQUIRE(N >= 128 && N % 128 == 0, PNPP_ERR_ARG, "%s: the row count N=%d must be a positive multiple of 128 (pad, and pass n_valid)", who, N);
    PNPP_REQUIRE(n_valid >= 1 && n_valid <= N, PNPP_ERR_ARG, "%s: n_valid=%d outside 1..N=%d", who, n_valid, N);
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "%s: B=%d exceeds the grid limit 65535", who, B);
    PNPP_REQUIRE(H <= 65535, PNPP_ERR_ARG, "%s: H=%d exceeds the grid limit 65535", who, H);
    return PNPP_OK;
}

}  // namespace
}  // namespace pnpp

using namespace pnpp;

extern "C" int pnpp_attention_infer_supported(int B, int N, int n_valid, int H, int head_dim) {
    return ai_check("attention_infer", B, N, n_valid, H, head_dim) == PNPP_OK ? 1 : 0;
}

// lengths == nullptr: the uniform call; otherwise the ragged one (pnpp_attention_infer_ragged refuses a null tensor before it comes here)
static int attention_infer_launch(const float *qkv, int B, int N, int n_valid, const int32_t *lengths, int H, int head_dim, float *out,
                                  void *stream) {
    PNPP_REQUIRE(qkv && out, PNPP_ERR_ARG, "attention_infer: null pointer");
    const int rc = ai_check("attention_infer", B, N, n_valid, H, head_dim);
    if (rc != PNPP_OK) return rc;
    ProfScope ps(as_stream(stream), lengths ? "attention_fwd_kernel<split> B=%d N=%d H=%d ragged=1" : "attention_fwd_kernel<split> B=%d N=%d H=%d", B, N, H);
    hipLaunchKernelGGL(attention_infer_kernel, dim3(N / 128, H, B), dim3(256), 0, as_stream(stream), qkv, N, n_valid, lengths, H, out);
    PNPP_CHECK_LAUNCH("attention_infer");
    return PNPP_OK;
}

extern "C" int pnpp_attention_infer(const float *qkv, int B, int N, int n_valid, int H, int head_dim, float *out, void *stream) {
    return attention_infer_launch(qkv, B, N, n_valid, nullptr, H, head_dim, out, stream);
}

extern "C" int pnpp_attention_infer_ragged(const float *qkv, int B, int N, int n_valid, const int32_t *lengths, int H, int head_dim, float *out,
                                           void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "attention_infer_ragged: null lengths pointer (the uniform call is pnpp_attention_infer)");
    return attention_infer_launch(qkv, B, N, n_valid, lengths, H, head_dim, out, stream);
}
