// gemm_smallm.h -- the body of the small-M GEMM as a device function, and the chunk constants it shares with the generic kernel.  The
// body runs as a kernel of its own (gemm_smallm_kernel, gemm_kernels.hip) and as the dA half of the launches that pair dA with dW
// (fc_dx_dw_kernel: gemm_kernels.hip; da_dw_kernel: dw_kernels.hip), which is why it is a header.
//
// Device code only, __forceinline__: no host code, nothing emitted on its own.
#pragma once
#include "operand_load.h"

namespace pnpp {

constexpr int KC = 32;       // reduction-dim chunk staged in LDS per step
constexpr int APITCH = KC + 1;  // odd pitch: the 32 rows a half-wave reads land on 32 different banks

// ---------------------------------------------------------------------------------------------
// small-M GEMM (fully connected head: M = batch rows).  One 32x32 output tile per workgroup; the
// reduction dimension is split over the 4 waves (chunk-interleaved), so a K=1024 layer is 8 chunks
// deep instead of 32.  A chunks go through wave-private LDS (row-major global -> lane-per-row
// operand), B (weights, [k][n] row-major) is read straight into the MFMA operand layout (the lane
// index is n: one 128-byte segment per half-wave).  Next chunk's loads fly during the MFMA loop.
// ---------------------------------------------------------------------------------------------
template <int AMODE, int EMODE, bool BT, int NW>
__device__ __forceinline__ void gemm_smallm_body(const AOperand &A, const BOperand &B, int M, int Nout, int Kd, const Epilogue &E,
                                                 int bx, int by, int nblocks) {
    // per wave: A chunk [32][33] and weight chunk [32 n][33] (BT only); after the K loop the first NW x 1024 floats
    // are reused for the K-split partials [NW][32][32] (a wave's partial overwrites only its own A chunk)
    constexpr int NTHR = NW * 64, NJ = 1024 / NTHR;
    __shared__ __attribute__((aligned(16))) float lds[2 * NW * 32 * APITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    float *As = lds + wave * 32 * APITCH;
    float *Ws = lds + (NW + wave) * 32 * APITCH;
    float *part = lds;  // [NW][32][32], wave w at part + w * 1056: inside its own A chunk region (32*33 = 1056 floats)
    const float *__restrict__ Bm = B.b;
    const int ldb = B.ldb;
    const int n0 = bx * 32, m0 = by * 32;
    const int nchunks = (Kd + KC - 1) / KC;
    const bool bvec = (ldb & 3) == 0 && ((uintptr_t)Bm & 15) == 0 && B.perm_D < 0 && B.rows >= 4 && (B.rows & 3) == 0;  // uniform

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    // E_BN_APPLY: the epilogue's per-column parameters and the dropout stream id are requested now -- behind the K loop and its
    // barriers each of them would be one more cold round trip (~1.5 us) on the tail of a 10 us launch
    float p_g = 1.f, p_b = 0.f, p_bias = 0.f, p_rm = 0.f, p_rv = 0.f;
    unsigned long long p_sid = 0ull;
    if constexpr (EMODE == E_BN_APPLY) {
        const BnTail &T = E.bn;
        if (tid < 32 && n0 + tid < Nout) {
            const int c = n0 + tid;
            if (T.gamma) p_g = T.gamma[c];
            if (T.beta) p_b = T.beta[c];
            if (T.bias) p_bias = T.bias[c];
            if (T.rm) p_rm = T.rm[c], p_rv = T.rv[c];
        }
        if (T.mask_out) p_sid = T.rng_counter[0];
    }

    RawA na[4];
    float4 nw[4];        // BT: weight rows, same (row, 4k) mapping as the A chunk
    float nb[KC / 2];    // !BT: weights already in operand layout
    auto fetch = [&](int c) {
        const int k0 = c * KC;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (lane >> 3) + 8 * i, k = k0 + 4 * (lane & 7);
            na[i] = fetch_a4<AMODE>(A, m0 + r, k, M, Kd);
            if constexpr (BT) {
                const float *wrow = Bm + (size_t)min(n0 + r, Nout - 1) * ldb;
                if (bvec) {
                    nw[i] = *reinterpret_cast<const float4 *>(wrow + min(k, B.rows - 4));
                } else {  // odd pitch or the layer-0 column permutation: four scalar loads (clamped; masked when staged)
                    float t[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int kp = min(k + e, B.rows - 1);
                        t[e] = wrow[B.perm_D >= 0 ? (kp < B.perm_D ? kp + 3 : kp - B.perm_D) : kp];
                    }
                    nw[i] = make_float4(t[0], t[1], t[2], t[3]);
                }
            }
        }
        if constexpr (!BT) {
#pragma unroll
            for (int s2 = 0; s2 < KC / 2; ++s2) {
                const int k = k0 + 2 * s2 + lh;
                // mask by multiplication, not by a select: hipcc turns "cond ? loaded : 0" into a branch around the load
                // with its own vmcnt(0), which serialises the sixteen operand loads of a chunk
                const float v = Bm[(size_t)min(k, B.rows - 1) * ldb + min(n0 + l31, Nout - 1)];
                nb[s2] = v * ((k < B.rows && n0 + l31 < Nout) ? 1.f : 0.f);
            }
        }
    };
    if (wave < nchunks) fetch(wave);
    for (int c = wave; c < nchunks; c += NW) {
        float cb[KC / 2];
        const int k0 = c * KC;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (lane >> 3) + 8 * i, k = k0 + 4 * (lane & 7);
            const int o = r * APITCH + 4 * (lane & 7);
            float v[4];
            xform_a4<AMODE>(A, na[i], m0 + r, k, M, Kd, v);
            As[o] = v[0], As[o + 1] = v[1], As[o + 2] = v[2], As[o + 3] = v[3];
            if constexpr (BT) {
                const bool okw = n0 + r < Nout;
                Ws[o] = (okw && k < B.rows) ? nw[i].x : 0.f;
                Ws[o + 1] = (okw && k + 1 < B.rows) ? nw[i].y : 0.f;
                Ws[o + 2] = (okw && k + 2 < B.rows) ? nw[i].z : 0.f;
                Ws[o + 3] = (okw && k + 3 < B.rows) ? nw[i].w : 0.f;
            }
        }
        if constexpr (!BT) {
#pragma unroll
            for (int s2 = 0; s2 < KC / 2; ++s2) cb[s2] = nb[s2];
        }
        if (c + NW < nchunks) fetch(c + NW);
#pragma unroll
        for (int s2 = 0; s2 < KC / 2; ++s2) {
            const float bv = BT ? Ws[l31 * APITCH + 2 * s2 + lh] : cb[s2];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[l31 * APITCH + 2 * s2 + lh], bv, acc, 0, 0, 0);
        }
    }
    // K-split reduction in fixed wave order, then the epilogue on the summed tile
#pragma unroll
    for (int r = 0; r < 16; ++r) part[wave * 32 * APITCH + ((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + l31] = acc[r];
    __syncthreads();
    float v[NJ], w2[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = tid + NTHR * j;
        v[j] = 0.f;
#pragma unroll
        for (int w = 0; w < NW; w += 4)  // groups of four waves, in wave order
            v[j] += (part[w * 32 * APITCH + e] + part[(w + 1) * 32 * APITCH + e]) +
                    (part[(w + 2) * 32 * APITCH + e] + part[(w + 3) * 32 * APITCH + e]);
        w2[j] = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = tid + NTHR * j, row = m0 + e / 32, col = n0 + e % 32;
        const bool ok = row < M && col < Nout;
        float x = ok ? v[j] : 0.f;
        if constexpr (EMODE == E_MASK_STATS) {
            const int cc = min(col, Nout - 1);
            const float zp = E.zp[(size_t)min(row, M - 1) * E.ldc + cc];
            x = (fmaf(zp, E.scale[cc], E.shift[cc]) > 0.f) ? x : 0.f;
            w2[j] = x * ((zp - E.mu[cc]) * E.istd[cc]);
            part[1024 + e] = w2[j];
        }
        part[e] = x;
        if (ok) E.c[(size_t)row * E.ldc + col] = x;
    }
    if constexpr (EMODE == E_BN_APPLY) {
        // the whole batch is in this tile: finish the BatchNorm here (same fp64 sums, in the same order, as the
        // slab + bn_finalize_fwd route), then normalise, ReLU and mask the tile
        const BnTail &T = E.bn;
        float *cs = part + 2048;  // [2][32] scale / shift of this column block
        __syncthreads();
        if (tid < 32 && n0 + tid < Nout) {
            const int c = n0 + tid;
            double s1 = 0.0, s2 = 0.0;
            for (int r = 0; r < 32; ++r) {
                const double x = (double)part[r * 32 + tid];
                s1 += x;
                s2 += x * x;
            }
            const double count = (double)M;
            const double mu = s1 / count;
            double var = s2 / count - mu * mu;
            if (var < 0.0) var = 0.0;
            const double is = 1.0 / sqrt(var + (double)T.eps);
            const double g = (double)p_g, bt = (double)p_b;
            const float sc = (float)(g * is), sh = (float)(bt - mu * g * is);
            T.mean[c] = (float)mu;
            T.istd[c] = (float)is;
            T.scale[c] = sc;
            T.shift[c] = sh;
            cs[tid] = sc;
            cs[32 + tid] = sh;
            if (T.rm) {
                const double bmean = mu + (double)p_bias;  // the linear bias was folded out of z
                const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
                T.rm[c] = (float)((1.0 - (double)T.momentum) * (double)p_rm + (double)T.momentum * bmean);
                T.rv[c] = (float)((1.0 - (double)T.momentum) * (double)p_rv + (double)T.momentum * unbiased);
            }
        }
        if (T.nbt && bx == 0 && tid == 0) *T.nbt += 1;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int e = tid + NTHR * j, row = m0 + e / 32, col = n0 + e % 32;
            if (row < M && col < Nout) {
                float y = fmaf(part[e], cs[e % 32], cs[32 + e % 32]);
                if (T.relu) y = fmaxf(y, 0.f);
                if (T.mask) y = T.mask[(size_t)row * E.ldc + col] ? y * T.drop_scale : 0.f;
                if (T.mask_out) {  // draw the keep bit of this element: one Philox word per element (a few hundred per workgroup)
                    const unsigned long long sid = p_sid;
                    const unsigned idx = (unsigned)(row * E.ldc + col);
                    unsigned c0 = idx, c1 = 0x44524f50u /* "DROP" */, c2 = (unsigned)sid, c3 = (unsigned)(sid >> 32);
                    unsigned k0 = (unsigned)T.rng_seed, k1 = (unsigned)(T.rng_seed >> 32);
#pragma unroll
                    for (int rd = 0; rd < 10; ++rd) {
                        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
                        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
                        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
                        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
                    }
                    const bool keep = (double)c0 >= (double)T.drop_p * 4294967296.0;
                    T.mask_out[(size_t)row * E.ldc + col] = keep ? 1 : 0;
                    y = keep ? y * T.drop_scale : 0.f;
                }
                T.y[(size_t)row * E.ldc + col] = y;
            }
        }
        if (T.mask_out) {  // every workgroup has read the counter above before it takes a ticket; the last one bumps it
            __syncthreads();
            if (tid == 0) {
                const unsigned long long t = atomicAdd(&T.rng_counter[1], 1ull);
                if (t == (unsigned long long)nblocks - 1) {
                    T.rng_counter[1] = 0ull;
                    T.rng_counter[0] += 1ull;
                }
            }
        }
    } else if constexpr (EMODE != E_STORE) {
        __syncthreads();
        if (tid < 32 && n0 + tid < Nout) {
            double s1 = 0.0, s2 = 0.0;
            for (int r = 0; r < 32; ++r) {
                const double x = (double)part[r * 32 + tid];
                s1 += x;
                if constexpr (EMODE == E_STORE_STATS) s2 += x * x;
                else s2 += (double)part[1024 + r * 32 + tid];
            }
            E.slab[((size_t)by * 2 + 0) * Nout + n0 + tid] = s1;
            E.slab[((size_t)by * 2 + 1) * Nout + n0 + tid] = s2;
        }
    }
}

}  // namespace pnpp
