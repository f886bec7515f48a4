// attention_train_kernels.hip -- the point transformer's TRAINING attention on the bf16 matrix pipe (pnpp_attention_split_fwd,
// pnpp_attention_split_bwd): what attention_fwd_kernel, attention_bwd_dq_kernel and attention_bwd_dkv_kernel (transformer_kernels.hip)
// compute, on the same buffers and under the same contract (qkv (B, N, 3E), N a multiple of 128, n_valid, head dimension 16, keep bits
// in both orientations, lse and dsum (B, H, N), padding rows of dqkv exact zeros, nothing a valid row receives depends on the padding,
// no atomics), with every matrix product on v_mfma_f32_32x32x16_bf16 from the exact three-way bf16 splits of its float32 operands
// (split_prims.h) in place of v_mfma_f32_32x32x2_f32.  The form is chosen by the entry point called; no environment switch.
// Ragged form (the _ragged entry points, `lengths` non-null): as in transformer_kernels.hip -- Nv is the cloud's own length (att_ragged_rows,
// common.h), out / lse / dQ rows beyond it are zeros, workgroups wholly beyond their cloud leave by blockIdx before any barrier.
//
// All three kernels: workgroup = 128 rows of one (cloud, head), 4 waves x 32 rows, a lane is a row (a query in the forward and dQ, a
// key in dK/dV) whose own operands are split once; the other side streams through LDS in stages of 64 rows (two 32-row tiles), double
// buffered, one barrier per stage, split into its three planes while it is staged, once per workgroup.
//
// Layouts (v_mfma_f32_32x32x16_bf16: lane 32 h + r holds A[row r][k = 8 h + j] and B[k = 8 h + j][column r], j = 0 .. 7;
// D[row (r & 3) + 8 (r >> 2) + 4 h][column = lane & 31] in register r).  Two LDS images of a staged 64 x 16 operand X:
//   row image   [dims 0..7 | dims 8..15][row][8]: the A fragment of X Y^T (contraction over the head dimension: one instruction per
//               partial product) is one 16-byte read.  The result tile has lane = this lane's row, register r = streamed row
//               kappa(r, h) = (r & 3) + 8 (r >> 2) + 4 h, as in the float32 kernels.
//   transposed  [dim][64 rows, pitch 72], the rows of a group of 16 stored in the order 4 h + j, 8 + 4 h + j: the A fragment of X^T W
//               whose B operand W is a tile held as above.  Step u takes the lane's registers 8 u .. 8 u + 7 as its B fragment, k = 8 h + j
//               naming streamed row kappa(8 u + j, h), so P, P keep and dS never move between lanes, and the A fragment is one 16-byte read
//               (the V^T image of attention_infer_kernels.hip).  Rows 16 .. 31 of X^T do not exist: lanes 16 .. 31 of a half-wave read the
//               fragment of dim (lane & 15), so rows 16 .. 31 of the result repeat rows 0 .. 15 and are never looked at.
//   K, Q and dO are needed in both images: the transposed one is written from the same split, as 2-byte stores.
//
// Softmax denominator: the sum of the UNDROPPED probabilities, formed on the VALU in the forward kernel, with or without keep bits --
// the "ones row of V^T" of the inference kernel would sum the P operand it is given, which under dropout is the dropped one.  The same
// instructions run in both cases, so lse does not depend on the mask, bit for bit.
//
// Products kept: all six of split_infer.h in every product (seven products: S, O; S, dP, dQ; S, dP, dV, dK), the leading one in its own
// accumulator (infer_chunk's comment says why); 1 / sqrt(16) is a power of two, so the split of the scaled Q stays exact.  DESIGN section
// 11 has the bound, the resource lines and the measurements.
#include "common.h"
#include "split_infer.h"

// As attention_infer_kernels.hip: ml = m * log2(e) must be ROUNDED, so that a row whose maximum did not move gets alpha = 1 exactly in
// the wave-uniform rescale branch.  The fused multiply-adds wanted are written fmaf.
#pragma clang fp contract(off)

namespace pnpp {
namespace {

constexpr int AT_DH = 16;                  // head dimension
constexpr int AT_ST = 64;                  // streamed rows per stage
constexpr int AT_RPLANE = 2 * AT_ST * 8;   // bf16 per plane of a row image: [2 dim halves][64 rows][8 dims]
constexpr int AT_TP = AT_ST + 8;           // pitch of a transposed image's row in bf16: 144 bytes, 16-byte reads of 16 consecutive rows hit every bank once
constexpr int AT_TPLANE = AT_DH * AT_TP;   // bf16 per plane of a transposed image
constexpr float AT_LOG2E = 1.4426950408889634f, AT_LN2 = 0.6931471805599453f;
constexpr float AT_SCALE = 0.25f;          // 1 / sqrt(AT_DH)

struct Frag3 {
    bf16x8 h, m, l;
};

// acc + accl += A B, the six products of split_infer.h
__device__ __forceinline__ void at_prod6(const Frag3 &a, const Frag3 &b, f32x16 &acc, f32x16 &accl) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, acc, 0, 0, 0);
    accl = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.h, accl, 0, 0, 0);
    accl = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.l, accl, 0, 0, 0);
    accl = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.m, accl, 0, 0, 0);
    accl = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.h, accl, 0, 0, 0);
    accl = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.m, accl, 0, 0, 0);
}
__device__ __forceinline__ f32x16 at_zero() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}
// X Y^T of one tile: A from planes of a row image (p points at plane 0, the planes are `plane` apart), B a lane's own fragment
__device__ __forceinline__ Frag3 at_ld3(const unsigned short *p, int plane) {
    Frag3 f;
    f.h = *reinterpret_cast<const bf16x8 *>(p), f.m = *reinterpret_cast<const bf16x8 *>(p + plane), f.l = *reinterpret_cast<const bf16x8 *>(p + 2 * plane);
    return f;
}
__device__ __forceinline__ f32x16 at_tile(const unsigned short *p, const Frag3 &b) {
    f32x16 s = at_zero(), sl = at_zero();
    at_prod6(at_ld3(p, AT_RPLANE), b, s, sl);
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] += sl[r];
    return s;
}
// eight floats, s * v each -> the fragment of a lane's own operand (k = 8 h + j = element j)
__device__ __forceinline__ Frag3 at_own(const float4 a, const float4 c, float s) {
    unsigned ph[4], pm[4], pl[4];
    sp_split2(a.x * s, a.y * s, ph[0], pm[0], pl[0]);
    sp_split2(a.z * s, a.w * s, ph[1], pm[1], pl[1]);
    sp_split2(c.x * s, c.y * s, ph[2], pm[2], pl[2]);
    sp_split2(c.z * s, c.w * s, ph[3], pm[3], pl[3]);
    Frag3 f;
    f.h = sp_frag(ph), f.m = sp_frag(pm), f.l = sp_frag(pl);
    return f;
}
// registers 8 u .. 8 u + 7 of a tile -> the B fragment of step u
__device__ __forceinline__ Frag3 at_regs(const f32x16 &s, int u) {
    unsigned ph[4], pm[4], pl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sp_split2(s[8 * u + 2 * i], s[8 * u + 2 * i + 1], ph[i], pm[i], pl[i]);
    Frag3 f;
    f.h = sp_frag(ph), f.m = sp_frag(pm), f.l = sp_frag(pl);
    return f;
}
// the streamed row kappa(r, h) a register of a tile belongs to
__device__ __forceinline__ constexpr int at_kappa(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// where row `row` (0 .. 63) of a stage sits in a row of the transposed image
__device__ __forceinline__ int at_tpos(int row) { return 16 * (row >> 4) + 8 * ((row >> 2) & 1) + 4 * ((row >> 3) & 1) + (row & 3); }

// Staging of a 64 x 16 operand by 256 threads: thread = (row tid >> 2, dims c4 .. c4 + 3), one float4, split once; `rimg` / `timg` point at
// plane 0 of the buffer's images (timg may be null: no transposed image).
struct Stager {
    int row, c4, rdst, tdst;
    __device__ __forceinline__ Stager(int tid) : row(tid >> 2), c4(4 * (tid & 3)) {
        rdst = (c4 >> 3) * (AT_ST * 8) + row * 8 + (c4 & 7);
        tdst = c4 * AT_TP + at_tpos(row);
    }
    __device__ __forceinline__ void put(const float4 v, float s, unsigned short *rimg, unsigned short *timg) const {
        unsigned a[3], c[3];
        sp_split2(v.x * s, v.y * s, a[0], a[1], a[2]);
        sp_split2(v.z * s, v.w * s, c[0], c[1], c[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            *reinterpret_cast<uint2 *>(rimg + p * AT_RPLANE + rdst) = make_uint2(a[p], c[p]);
            if (timg) {
                unsigned short *t = timg + p * AT_TPLANE + tdst;
                t[0] = (unsigned short)a[p], t[AT_TP] = (unsigned short)(a[p] >> 16);
                t[2 * AT_TP] = (unsigned short)c[p], t[3 * AT_TP] = (unsigned short)(c[p] >> 16);
            }
        }
    }
};

// ---- forward: attention_infer_kernel's tiling, plus lse and the keep bits --------------------------------------------------------------
__global__ void __launch_bounds__(256, 3)   // the row sum, lse and the keep words do not fit the inference kernel's 128 registers without scratch (72 bytes at four waves)
attention_train_fwd_kernel(const float *__restrict__ qkv, int N, int Nv, const int *__restrict__ lengths, int H,
                           const unsigned *__restrict__ mask, float keep_scale, float *__restrict__ out, float *__restrict__ lse) {
    __shared__ __attribute__((aligned(16))) unsigned short Ks[2][3][AT_RPLANE];
    __shared__ __attribute__((aligned(16))) unsigned short Vs[2][3][AT_TPLANE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z, E = H * AT_DH, ld = 3 * E;
    const float *base = qkv + (size_t)b * N * ld;
    const int q = blockIdx.x * 128 + wave * 32 + l31;   // this lane's query (N % 128 == 0: the row exists)
    const int Nz = att_ragged_rows(lengths, b, N, Nv);  // ragged form: Nv becomes the cloud's own length, rows from Nz on are written as zeros
    if ((int)blockIdx.x * 128 >= Nz) {                  // a workgroup wholly beyond its cloud (by blockIdx: all of it leaves before any barrier)
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 *orow = reinterpret_cast<float4 *>(out + ((size_t)b * N + q) * E + h * AT_DH + 4 * lh);
        orow[0] = z, orow[2] = z;
        if (lse && lh == 0) lse[((size_t)b * H + h) * N + q] = 0.f;
        return;
    }

    Frag3 qf;   // Q^T operand: dims 8 h .. 8 h + 7 of this lane's query, scaled
    {
        const float4 *qp = reinterpret_cast<const float4 *>(base + (size_t)q * ld + h * AT_DH + 8 * lh);
        qf = at_own(qp[0], qp[1], AT_SCALE);
    }
    // staging map.  K: the Stager's.  V: thread = (dim, four consecutive keys), so that the split leaves a run of four keys of one dim
    // per plane: one 8-byte write into the key-contiguous image (as attention_infer_kernel).
    const Stager ks(tid);
    const float *k_src = base + E + h * AT_DH + ks.c4 + (size_t)ks.row * ld;
    const int v_dim = tid & 15, v_kg = tid >> 4;
    const float *v_src = base + 2 * E + h * AT_DH + v_dim + (size_t)(4 * v_kg) * ld;
    const int v_dst = v_dim * AT_TP + at_tpos(4 * v_kg);
    const unsigned *m_src = mask ? mask + (((size_t)b * H + h) * N + q) * (N / 32) : nullptr;   // this query's keep words, 32 keys each
    float4 kf;
    float vf[4];
    uint2 mw = make_uint2(0xffffffffu, 0xffffffffu), mw_next = mw;
    auto fetch = [&](int st) {   // rows st * 64 .. + 63 exist: the stages cover ceil(Nv / 64) * 64 <= N rows
        const size_t row = (size_t)st * AT_ST * ld;
        kf = *reinterpret_cast<const float4 *>(k_src + row);
#pragma unroll
        for (int i = 0; i < 4; ++i) vf[i] = v_src[row + (size_t)i * ld];
        if (m_src) mw_next = *reinterpret_cast<const uint2 *>(m_src + 2 * st);   // a 64-key stage is two words
    };
    auto put = [&](int buf) {
        ks.put(kf, 1.f, &Ks[buf][0][0], nullptr);
        unsigned a[3], c[3];
        sp_split2(vf[0], vf[1], a[0], a[1], a[2]);
        sp_split2(vf[2], vf[3], c[0], c[1], c[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2 *>(&Vs[buf][p][v_dst]) = make_uint2(a[p], c[p]);
    };

    f32x16 o = at_zero(), ol = at_zero();   // O^T: the leading products and the five small ones
    float m_run = -INFINITY, ml_run = -INFINITY, l_run = 0.f;   // running row maximum, the same times log2(e) as it is rounded, row sum

    const int nst = (Nv + AT_ST - 1) / AT_ST;
    fetch(0);
    put(0);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        mw = mw_next;
        if (st + 1 < nst) fetch(st + 1);   // in flight while this stage is computed
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k0 = st * AT_ST + 32 * t;
            if (k0 >= Nv) break;   // a key block without a point
            f32x16 s = at_tile(&Ks[buf][0][lh * (AT_ST * 8) + (32 * t + l31) * 8], qf);
            if (k0 + 32 > Nv) {   // the last block of a cloud whose size is not a multiple of 32
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = k0 + at_kappa(r, lh) < Nv ? s[r] : -INFINITY;
            }
            float mx = s[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (__builtin_amdgcn_ballot_w64(mx > m_run) != 0ull) {   // wave-uniform: no row maximum moved, nothing to rescale
                const float m_new = fmaxf(m_run, mx), ml_new = m_new * AT_LOG2E;
                const float alpha = __builtin_amdgcn_exp2f(ml_run - ml_new);   // exp2(-inf) = 0 on the first block; 1 for a row that did not move
#pragma unroll
                for (int r = 0; r < 8; ++r) o[r] *= alpha, ol[r] *= alpha;
                l_run *= alpha;
                m_run = m_new, ml_run = ml_new;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], AT_LOG2E, -ml_run));
            // the softmax normalisation is over the undropped weights: summed here, before the keep bits, in one fixed order
            float rs = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
            rs += ((s[8] + s[9]) + (s[10] + s[11])) + ((s[12] + s[13]) + (s[14] + s[15]));
            rs += __shfl_xor(rs, 32, 64);
            l_run += rs;
            if (mask) {   // dropout on the weights: keep bit of (query, key kappa(r, h)), scaled by 1 / (1 - p)
                const unsigned w = t ? mw.y : mw.x;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = ((w >> at_kappa(r, lh)) & 1u) ? s[r] * keep_scale : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
                at_prod6(at_ld3(&Vs[buf][0][(l31 & 15) * AT_TP + (2 * t + u) * 16 + lh * 8], AT_TPLANE), at_regs(s, u), o, ol);
        }
        if (st + 1 < nst) put(buf ^ 1);   // the other buffer was last read before the previous barrier
        __syncthreads();
    }
    const float inv = 1.f / l_run;
    float tr[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) tr[r] = q < Nz ? (o[r] + ol[r]) * inv : 0.f;
    float4 *orow = reinterpret_cast<float4 *>(out + ((size_t)b * N + q) * E + h * AT_DH + 4 * lh);
    orow[0] = make_float4(tr[0], tr[1], tr[2], tr[3]);   // dims 4 h + 0 .. 3
    orow[2] = make_float4(tr[4], tr[5], tr[6], tr[7]);   // dims 8 + 4 h + 0 .. 3
    // natural log, although the loop works in the log2 domain: the probabilities are exp2(s log2(e) - ml) with ml the ROUNDED m log2(e),
    // so their sum is that of exp(s - m) times exp2(m log2(e) - ml); the residual is exact in one fma
    if (lse && lh == 0) lse[((size_t)b * H + h) * N + q] = q < Nz ? m_run + (logf(l_run) - fmaf(m_run, AT_LOG2E, -ml_run) * AT_LN2) : 0.f;
}

// ---- dQ: a wave owns 32 queries and walks the keys.  S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (keep dP^T - D), dQ^T += K^T dS^T ---------------
__global__ void __launch_bounds__(256, 2)
attention_train_dq_kernel(const float *__restrict__ qkv, const float *__restrict__ o, const float *__restrict__ d_o,
                          const float *__restrict__ lse, int N, int Nv, const int *__restrict__ lengths, int H,
                          const unsigned *__restrict__ mask, float keep_scale, float *__restrict__ dqkv, float *__restrict__ dsum) {
    __shared__ __attribute__((aligned(16))) unsigned short Kr[2][3][AT_RPLANE], Vr[2][3][AT_RPLANE];
    __shared__ __attribute__((aligned(16))) unsigned short Kt[2][3][AT_TPLANE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z, E = H * AT_DH, ld = 3 * E;
    const float *base = qkv + (size_t)b * N * ld;
    const int q = blockIdx.x * 128 + wave * 32 + l31;
    const int Nz = att_ragged_rows(lengths, b, N, Nv);
    if ((int)blockIdx.x * 128 >= Nz) {   // wholly beyond the cloud: zero dQ rows (dsum of these rows is never read: the dK/dV kernel skips them)
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 *drow = reinterpret_cast<float4 *>(dqkv + ((size_t)b * N + q) * ld + h * AT_DH + 4 * lh);
        drow[0] = z, drow[2] = z;
        return;
    }

    Frag3 qf, gf;   // this lane's query and its dO row, dims 8 h .. 8 h + 7, split once
    float D;
    {
        const float4 *qp = reinterpret_cast<const float4 *>(base + (size_t)q * ld + h * AT_DH + 8 * lh);
        qf = at_own(qp[0], qp[1], AT_SCALE);
        const size_t at = ((size_t)b * N + q) * E + h * AT_DH + 8 * lh;
        const float4 *gp = reinterpret_cast<const float4 *>(d_o + at), *op = reinterpret_cast<const float4 *>(o + at);
        const float4 g0 = gp[0], g1 = gp[1], o0 = op[0], o1 = op[1];
        gf = at_own(g0, g1, 1.f);
        float dpart = g0.x * o0.x;
        dpart = fmaf(g0.y, o0.y, dpart), dpart = fmaf(g0.z, o0.z, dpart), dpart = fmaf(g0.w, o0.w, dpart);
        dpart = fmaf(g1.x, o1.x, dpart), dpart = fmaf(g1.y, o1.y, dpart), dpart = fmaf(g1.z, o1.z, dpart), dpart = fmaf(g1.w, o1.w, dpart);
        D = dpart + __shfl_xor(dpart, 32, 64);
    }
    const float L = lse[((size_t)b * H + h) * N + q];
    if (lh == 0) dsum[((size_t)b * H + h) * N + q] = D;

    const Stager sg(tid);
    const float *k_src = base + E + h * AT_DH + sg.c4 + (size_t)sg.row * ld, *v_src = k_src + E;
    const unsigned *m_src = mask ? mask + (((size_t)b * H + h) * N + q) * (N / 32) : nullptr;
    float4 kf, vf;
    uint2 mw = make_uint2(0xffffffffu, 0xffffffffu), mw_next = mw;
    auto fetch = [&](int st) {   // rows st * 64 .. + 63 exist: the stages cover ceil(Nv / 64) * 64 <= N rows
        const size_t row = (size_t)st * AT_ST * ld;
        kf = *reinterpret_cast<const float4 *>(k_src + row);
        vf = *reinterpret_cast<const float4 *>(v_src + row);
        if (m_src) mw_next = *reinterpret_cast<const uint2 *>(m_src + 2 * st);
    };
    auto put = [&](int buf) {
        sg.put(kf, 1.f, &Kr[buf][0][0], &Kt[buf][0][0]);
        sg.put(vf, 1.f, &Vr[buf][0][0], nullptr);
    };

    f32x16 dq = at_zero(), dql = at_zero();
    const int nst = (Nv + AT_ST - 1) / AT_ST;   // keys beyond the cloud's Nv points carry no weight (P = 0)
    fetch(0);
    put(0);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        mw = mw_next;
        if (st + 1 < nst) fetch(st + 1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k0 = st * AT_ST + 32 * t;
            if (k0 >= Nv) break;
            const int roff = lh * (AT_ST * 8) + (32 * t + l31) * 8;
            f32x16 s = at_tile(&Kr[buf][0][roff], qf);    // S^T  = K Q^T
            f32x16 dp = at_tile(&Vr[buf][0][roff], gf);   // dP^T = V dO^T
            if (mask) {   // d(dropped weights) -> d(weights): the same keep bits and scale as the forward
                const unsigned w = t ? mw.y : mw.x;
#pragma unroll
                for (int r = 0; r < 16; ++r) dp[r] = ((w >> at_kappa(r, lh)) & 1u) ? dp[r] * keep_scale : 0.f;
            }
            if (k0 + 32 > Nv) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = k0 + at_kappa(r, lh) < Nv ? s[r] : -INFINITY;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = __expf(s[r] - L) * (dp[r] - D);   // dS^T = P^T * (dP^T - D)
#pragma unroll
            for (int u = 0; u < 2; ++u)
                at_prod6(at_ld3(&Kt[buf][0][(l31 & 15) * AT_TP + (2 * t + u) * 16 + lh * 8], AT_TPLANE), at_regs(s, u), dq, dql);
        }
        if (st + 1 < nst) put(buf ^ 1);
        __syncthreads();
    }
    float tr[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) tr[r] = q < Nz ? (dq[r] + dql[r]) * AT_SCALE : 0.f;
    float4 *drow = reinterpret_cast<float4 *>(dqkv + ((size_t)b * N + q) * ld + h * AT_DH + 4 * lh);
    drow[0] = make_float4(tr[0], tr[1], tr[2], tr[3]);
    drow[2] = make_float4(tr[4], tr[5], tr[6], tr[7]);
}

// ---- dK, dV: a wave owns 32 keys and walks the query blocks.  S = (scale Q) K^T, dP = dO V^T, dV^T += dO^T (P keep), dK^T += (scale Q)^T dS ----
__global__ void __launch_bounds__(256, 2)
attention_train_dkv_kernel(const float *__restrict__ qkv, const float *__restrict__ d_o, const float *__restrict__ lse,
                           const float *__restrict__ dsum, int N, int Nv, const int *__restrict__ lengths, int H,
                           const unsigned *__restrict__ maskT, float keep_scale, float *__restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) unsigned short Qr[2][3][AT_RPLANE], Gr[2][3][AT_RPLANE];
    __shared__ __attribute__((aligned(16))) unsigned short Qt[2][3][AT_TPLANE], Gt[2][3][AT_TPLANE];
    __shared__ __attribute__((aligned(16))) float Ls[2][AT_ST], Ds[2][AT_ST];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z, E = H * AT_DH, ld = 3 * E;
    const float *base = qkv + (size_t)b * N * ld;
    const int key = blockIdx.x * 128 + wave * 32 + l31;
    if ((int)blockIdx.x * 128 >= att_ragged_rows(lengths, b, N, Nv)) {   // every key of the workgroup is padding: zero rows, no walk over the queries
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        float *drow = dqkv + ((size_t)b * N + key) * ld + h * AT_DH + 4 * lh;
        float4 *krow = reinterpret_cast<float4 *>(drow + E), *vrow = reinterpret_cast<float4 *>(drow + 2 * E);
        krow[0] = z, krow[2] = z, vrow[0] = z, vrow[2] = z;
        return;
    }
    const bool kvalid = key < Nv;

    Frag3 kf3, vf3;   // this lane's key and value rows, split once.  A padding key's are taken as zeros: what its row holds is never used
    {
        const float4 *kp = reinterpret_cast<const float4 *>(base + (size_t)key * ld + E + h * AT_DH + 8 * lh);
        const float4 *vp = reinterpret_cast<const float4 *>(base + (size_t)key * ld + 2 * E + h * AT_DH + 8 * lh);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        kf3 = at_own(kvalid ? kp[0] : z, kvalid ? kp[1] : z, 1.f);
        vf3 = at_own(kvalid ? vp[0] : z, kvalid ? vp[1] : z, 1.f);
    }
    // staging: the (scaled) query tile and the dO tile, both images each; threads 0 .. 63 / 64 .. 127 also L / D
    const Stager sg(tid);
    const float *q_src = base + h * AT_DH + sg.c4 + (size_t)sg.row * ld;
    const float *g_src = d_o + (size_t)b * N * E + h * AT_DH + sg.c4 + (size_t)sg.row * E;
    const float *ld_src = tid < AT_ST ? lse + ((size_t)b * H + h) * N + tid : dsum + ((size_t)b * H + h) * N + (tid & (AT_ST - 1));
    const unsigned *m_src = maskT ? maskT + (((size_t)b * H + h) * N + key) * (N / 32) : nullptr;   // this key's keep words, 32 queries each
    float4 qf, gf;
    float ldv = 0.f;
    uint2 mw = make_uint2(0xffffffffu, 0xffffffffu), mw_next = mw;
    auto fetch = [&](int st) {   // rows st * 64 .. + 63 exist: the stages cover ceil(Nv / 64) * 64 <= N rows
        qf = *reinterpret_cast<const float4 *>(q_src + (size_t)st * AT_ST * ld);
        gf = *reinterpret_cast<const float4 *>(g_src + (size_t)st * AT_ST * E);
        if (tid < 2 * AT_ST) ldv = ld_src[st * AT_ST];
        if (m_src) mw_next = *reinterpret_cast<const uint2 *>(m_src + 2 * st);
    };
    auto put = [&](int buf) {
        sg.put(qf, AT_SCALE, &Qr[buf][0][0], &Qt[buf][0][0]);
        sg.put(gf, 1.f, &Gr[buf][0][0], &Gt[buf][0][0]);
        if (tid < AT_ST) Ls[buf][tid] = ldv;
        else if (tid < 2 * AT_ST) Ds[buf][tid - AT_ST] = ldv;
    };

    f32x16 dk = at_zero(), dkl = at_zero(), dv = at_zero(), dvl = at_zero();
    // queries beyond the cloud's Nv points are padding: their dO is zero, so they add nothing and their blocks are skipped
    const int nst = (Nv + AT_ST - 1) / AT_ST;
    fetch(0);
    put(0);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        mw = mw_next;
        if (st + 1 < nst) fetch(st + 1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int q0 = st * AT_ST + 32 * t;
            if (q0 >= Nv) break;
            const int roff = lh * (AT_ST * 8) + (32 * t + l31) * 8;
            f32x16 s = at_tile(&Qr[buf][0][roff], kf3);    // S  = (scale Q) K^T
            f32x16 dp = at_tile(&Gr[buf][0][roff], vf3);   // dP = dO V^T
            const unsigned w = t ? mw.y : mw.x;
#pragma unroll
            for (int c = 0; c < 4; ++c) {   // registers 4 c .. 4 c + 3 are queries 8 c + 4 h + 0 .. 3: one 16-byte read each of L and D
                const float4 l4 = *reinterpret_cast<const float4 *>(&Ls[buf][32 * t + 8 * c + 4 * lh]);
                const float4 d4 = *reinterpret_cast<const float4 *>(&Ds[buf][32 * t + 8 * c + 4 * lh]);
                const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 4 * c + i;
                    const float keep = ((w >> at_kappa(r, lh)) & 1u) ? keep_scale : 0.f;
                    const float pr = __expf(s[r] - lq[i]);      // P
                    dp[r] = pr * (dp[r] * keep - dq4[i]);       // dS = P * (d(dropped P) * keep / (1 - p) - D)
                    s[r] = pr * keep;                           // dropped P, the operand of dV
                }
            }
            if (q0 + 32 > Nv) {   // the cloud's last, partial query block: padding queries contribute nothing
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool qv = q0 + at_kappa(r, lh) < Nv;
                    dp[r] = qv ? dp[r] : 0.f, s[r] = qv ? s[r] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int toff = (l31 & 15) * AT_TP + (2 * t + u) * 16 + lh * 8;
                at_prod6(at_ld3(&Gt[buf][0][toff], AT_TPLANE), at_regs(s, u), dv, dvl);    // dV^T += dO^T P
                at_prod6(at_ld3(&Qt[buf][0][toff], AT_TPLANE), at_regs(dp, u), dk, dkl);   // dK^T += (scale Q)^T dS
            }
        }
        if (st + 1 < nst) put(buf ^ 1);
        __syncthreads();
    }
    // padding keys took no part in the forward softmax: their rows are written as zeros -- selected, not multiplied by 0
    float tk[8], tv[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) tk[r] = kvalid ? dk[r] + dkl[r] : 0.f, tv[r] = kvalid ? dv[r] + dvl[r] : 0.f;
    float *drow = dqkv + ((size_t)b * N + key) * ld + h * AT_DH + 4 * lh;
    float4 *krow = reinterpret_cast<float4 *>(drow + E), *vrow = reinterpret_cast<float4 *>(drow + 2 * E);
    krow[0] = make_float4(tk[0], tk[1], tk[2], tk[3]);
    krow[2] = make_float4(tk[4], tk[5], tk[6], tk[7]);
    vrow[0] = make_float4(tv[0], tv[1], tv[2], tv[3]);
    vrow[2] = make_float4(tv[4], tv[5], tv[6], tv[7]);
}

int at_check(const char *who, int B, int N, int n_valid, int H, int head_dim) {
    PNPP_REQUIRE(B >= 1, PNPP_ERR_ARG, "%s: B=%d, at least one cloud is needed", who, B);
    PNPP_REQUIRE(H >= 1, PNPP_ERR_ARG, "%s: H=%d, at least one head is needed", who, H);
    PNPP_REQUIRE(head_dim == AT_DH, PNPP_ERR_ARG, "%s: head_dim=%d is not supported (only %d)", who, head_dim, AT_DH);
    PNPP_REQUIRE(N >= 128 && N % 128 == 0, PNPP_ERR_ARG, "%s: the row count N=%d must be a positive multiple of 128 (pad, and pass n_valid)", who, N);
    PNPP_REQUIRE(n_valid >= 1 && n_valid <= N, PNPP_ERR_ARG, "%s: n_valid=%d outside 1..N=%d", who, n_valid, N);
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "%s: B=%d exceeds the grid limit 65535", who, B);
    PNPP_REQUIRE(H <= 65535, PNPP_ERR_ARG, "%s: H=%d exceeds the grid limit 65535", who, H);
    return PNPP_OK;
}

}  // namespace
}  // namespace pnpp

using namespace pnpp;

extern "C" int pnpp_attention_split_supported(int B, int N, int n_valid, int H, int head_dim) {
    return at_check("attention_split", B, N, n_valid, H, head_dim) == PNPP_OK ? 1 : 0;
}

// lengths == nullptr: the uniform call; otherwise the ragged one (the _ragged entry points refuse a null tensor before they come here)
static int attention_split_fwd_launch(const float *qkv, int B, int N, int n_valid, const int32_t *lengths, int H, int head_dim,
                                      const uint32_t *mask, float p, float *out, float *lse, void *stream) {
    PNPP_REQUIRE(qkv && out, PNPP_ERR_ARG, "attention_split_fwd: null pointer");
    const int rc = at_check("attention_split_fwd", B, N, n_valid, H, head_dim);
    if (rc != PNPP_OK) return rc;
    PNPP_REQUIRE(p >= 0.f && p < 1.f, PNPP_ERR_ARG, "attention_split_fwd: dropout p=%g outside [0, 1)", (double)p);
    ProfScope ps(as_stream(stream), lengths ? "attention_fwd_kernel<split,train> B=%d N=%d H=%d ragged=1" : "attention_fwd_kernel<split,train> B=%d N=%d H=%d",
                 B, N, H);
    hipLaunchKernelGGL(attention_train_fwd_kernel, dim3(N / 128, H, B), dim3(256), 0, as_stream(stream), qkv, N, n_valid, lengths, H, mask,
                       1.0f / (1.0f - p), out, lse);
    PNPP_CHECK_LAUNCH("attention_split_fwd");
    return PNPP_OK;
}

extern "C" int pnpp_attention_split_fwd(const float *qkv, int B, int N, int n_valid, int H, int head_dim, const uint32_t *mask, float p,
                                        float *out, float *lse, void *stream) {
    return attention_split_fwd_launch(qkv, B, N, n_valid, nullptr, H, head_dim, mask, p, out, lse, stream);
}

extern "C" int pnpp_attention_split_fwd_ragged(const float *qkv, int B, int N, int n_valid, const int32_t *lengths, int H, int head_dim,
                                               const uint32_t *mask, float p, float *out, float *lse, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "attention_split_fwd_ragged: null lengths pointer (the uniform call is pnpp_attention_split_fwd)");
    return attention_split_fwd_launch(qkv, B, N, n_valid, lengths, H, head_dim, mask, p, out, lse, stream);
}

static int attention_split_bwd_launch(const float *qkv, const float *out, const float *d_out, const float *lse, int B, int N, int n_valid,
                                      const int32_t *lengths, int H, int head_dim, const uint32_t *mask, const uint32_t *maskT, float p,
                                      float *dqkv, float *dsum, void *stream) {
    PNPP_REQUIRE((mask == nullptr) == (maskT == nullptr), PNPP_ERR_ARG, "attention_split_bwd: pass both mask orientations or neither");
    PNPP_REQUIRE(p >= 0.f && p < 1.f, PNPP_ERR_ARG, "attention_split_bwd: dropout p=%g outside [0, 1)", (double)p);
    PNPP_REQUIRE(qkv && out && d_out && lse && dqkv && dsum, PNPP_ERR_ARG, "attention_split_bwd: null pointer");
    const int rc = at_check("attention_split_bwd", B, N, n_valid, H, head_dim);
    if (rc != PNPP_OK) return rc;
    const float keep_scale = 1.0f / (1.0f - p);
    hipStream_t st = as_stream(stream);
    {
        ProfScope ps(st, lengths ? "attention_bwd_dq_kernel<split> B=%d N=%d H=%d ragged=1" : "attention_bwd_dq_kernel<split> B=%d N=%d H=%d", B, N, H);
        hipLaunchKernelGGL(attention_train_dq_kernel, dim3(N / 128, H, B), dim3(256), 0, st, qkv, out, d_out, lse, N, n_valid, lengths, H, mask,
                           keep_scale, dqkv, dsum);
        PNPP_CHECK_LAUNCH("attention_split_bwd_dq");
    }
    {
        ProfScope ps(st, lengths ? "attention_bwd_dkv_kernel<split> B=%d N=%d H=%d ragged=1" : "attention_bwd_dkv_kernel<split> B=%d N=%d H=%d", B, N, H);
        hipLaunchKernelGGL(attention_train_dkv_kernel, dim3(N / 128, H, B), dim3(256), 0, st, qkv, d_out, lse, dsum, N, n_valid, lengths, H, maskT,
                           keep_scale, dqkv);
        PNPP_CHECK_LAUNCH("attention_split_bwd_dkv");
    }
    return PNPP_OK;
}

extern "C" int pnpp_attention_split_bwd(const float *qkv, const float *out, const float *d_out, const float *lse, int B, int N, int n_valid,
                                        int H, int head_dim, const uint32_t *mask, const uint32_t *maskT, float p, float *dqkv, float *dsum,
                                        void *stream) {
    return attention_split_bwd_launch(qkv, out, d_out, lse, B, N, n_valid, nullptr, H, head_dim, mask, maskT, p, dqkv, dsum, stream);
}

extern "C" int pnpp_attention_split_bwd_ragged(const float *qkv, const float *out, const float *d_out, const float *lse, int B, int N,
                                               int n_valid, const int32_t *lengths, int H, int head_dim, const uint32_t *mask,
                                               const uint32_t *maskT, float p, float *dqkv, float *dsum, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "attention_split_bwd_ragged: null lengths pointer (the uniform call is pnpp_attention_split_bwd)");
    return attention_split_bwd_launch(qkv, out, d_out, lse, B, N, n_valid, lengths, H, head_dim, mask, maskT, p, dqkv, dsum, stream);
}
