// fc_kernels.hip -- kernels of the fully connected block Linear -> {BatchNorm1d | LayerNorm | none} -> ReLU -> dropout
// (models/pointnet_pp_vonMises.py:32-35, pointnet_pp_8dir.py:81-85, pointnet_pp_mvM.py:82-83,91-122) and one launch_fc_* per
// kernel (csrc/fc.h): the launcher owns the kernel's grid, its LDS size, its ProfScope tag and its launch-check label.  Which of
// them a call takes is decided in csrc/fc_api.hip.
//
// The matrix products run on the same fused MFMA GEMM / dW kernels as the set-abstraction layers;
// the row/column normalisation passes here touch only M x N elements (M = batch), so they are plain
// wave-per-row / lane-per-column kernels with float64 accumulation.
#include "fc.h"
#include "launch.h"

namespace pnpp {

// y = dropout(relu(z*scale + shift))   (BatchNorm) or   y = dropout(relu(z + b))   (no norm)
__global__ void __launch_bounds__(256) fc_apply_cols_kernel(const float *__restrict__ z, const float *__restrict__ scale,
                                                            const float *__restrict__ shift, const uint8_t *__restrict__ mask,
                                                            float drop_scale, int relu, int M, int N, float *__restrict__ y) {
    const size_t total = (size_t)M * N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int n = (int)(i % N);
        float v = fmaf(z[i], scale ? scale[n] : 1.f, shift[n]);
        if (relu) v = fmaxf(v, 0.f);
        if (mask) v = mask[i] ? v * drop_scale : 0.f;
        y[i] = v;
    }
}

// keep-bit of element idx of the dropout draw with stream id sid: one Philox4x32-10 word per element, exactly the draw of the
// BatchNorm epilogue (gemm_smallm_body, E_BN_APPLY) -- counter (idx, "DROP", sid), key = seed
__device__ __forceinline__ bool dropout_keep(unsigned idx, unsigned long long sid, unsigned long long seed, float drop_p) {
    unsigned c0 = idx, c1 = 0x44524f50u /* "DROP" */, c2 = (unsigned)sid, c3 = (unsigned)(sid >> 32);
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int rd = 0; rd < 10; ++rd) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return (double)c0 >= (double)drop_p * 4294967296.0;
}

// LayerNorm over the feature axis of u = z + b; one 256-thread block per row.  mask_out (round 4): the keep-mask of nn.Dropout is
// DRAWN here (no RNG launch, graph-replayable: the stream id lives in device memory, rng_counter[0], and is bumped by the last row
// block through the ticket word rng_counter[1]) and written out for the backward pass
__global__ void __launch_bounds__(256) fc_apply_ln_kernel(const float *__restrict__ z, const float *__restrict__ b,
                                                          const float *__restrict__ nw, const float *__restrict__ nb,
                                                          const uint8_t *__restrict__ mask, float drop_scale, int relu, int N,
                                                          float eps, float *__restrict__ y, float *__restrict__ mean,
                                                          float *__restrict__ istd, uint8_t *__restrict__ mask_out, float drop_p,
                                                          unsigned long long rng_seed, unsigned long long *__restrict__ rng_counter) {
    __shared__ double red[2][4];
    const int m = blockIdx.x;
    const unsigned long long sid = mask_out ? rng_counter[0] : 0ull;   // requested before the reductions
    const float *zr = z + (size_t)m * N;
    double s1 = 0.0, s2 = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const double u = (double)zr[n] + (double)b[n];
        s1 += u;
        s2 += u * u;
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s1 += shfl_xor_f64(s1, k), s2 += shfl_xor_f64(s2, k);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = s1, red[1][threadIdx.x >> 6] = s2;
    __syncthreads();
    s1 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    s2 = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const double mu = s1 / N;
    double var = s2 / N - mu * mu;
    if (var < 0.0) var = 0.0;
    const double is = 1.0 / sqrt(var + (double)eps);
    if (threadIdx.x == 0) mean[m] = (float)mu, istd[m] = (float)is;
    const float muf = (float)mu, isf = (float)is;
    for (int n = threadIdx.x; n < N; n += 256) {
        float v = ((zr[n] + b[n]) - muf) * isf * nw[n] + nb[n];
        if (relu) v = fmaxf(v, 0.f);
        if (mask) v = mask[(size_t)m * N + n] ? v * drop_scale : 0.f;
        if (mask_out) {
            const bool keep = dropout_keep((unsigned)(m * N + n), sid, rng_seed, drop_p);
            mask_out[(size_t)m * N + n] = keep ? 1 : 0;
            v = keep ? v * drop_scale : 0.f;
        }
        y[(size_t)m * N + n] = v;
    }
    if (mask_out) {   // every row block has read the stream id above before it takes a ticket; the last one bumps it
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long t = atomicAdd(&rng_counter[1], 1ull);
            if (t == (unsigned long long)gridDim.x - 1) {
                rng_counter[1] = 0ull;
                rng_counter[0] += 1ull;
            }
        }
    }
}

// ---- backward, BatchNorm1d / none: block = 32 columns x 8 row lanes --------------------------------
// g = dy * dropout * relu'; BN: dz = gamma*istd*(g - mean(g) - xhat*mean(g*xhat)); none: dz = g
// Row-parallel form of the plain (no normalisation) case for many rows (the per-point linear layers of the transformer,
// M = B * N): dz = dy with the dropout mask and the ReLU gate applied, and one [N] partial of the bias gradient per
// 256-row chunk (slab_reduce adds them).  grid = (N / 64 column blocks, M / 256 row chunks).
__global__ void __launch_bounds__(256)
fc_bwd_rows_kernel(const float *__restrict__ dy, const float *__restrict__ z, const uint8_t *__restrict__ mask, float drop_scale,
                   int relu, const float *__restrict__ bias, int M, int N, float *__restrict__ dz, float *__restrict__ slab) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + cl, m0 = blockIdx.y * 256;
    const float sh = n < N ? bias[n] : 0.f;
    float acc = 0.f;
    if (n < N)
        for (int r = rl; r < 256; r += 4) {
            const int m = m0 + r;
            if (m >= M) break;
            const size_t i = (size_t)m * N + n;
            float g = dy[i];
            if (mask) g = mask[i] ? g * drop_scale : 0.f;
            if (relu && !(z[i] + sh > 0.f)) g = 0.f;
            dz[i] = g;
            acc += g;
        }
    red[rl][cl] = acc;
    __syncthreads();
    if (rl == 0 && n < N) slab[(size_t)blockIdx.y * N + n] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

__global__ void __launch_bounds__(256)
fc_bwd_cols_kernel(const float *__restrict__ dy, const float *__restrict__ z, const uint8_t *__restrict__ mask,
                   float drop_scale, int relu, int bn, const float *__restrict__ scale, const float *__restrict__ shift,
                   const float *__restrict__ mean, const float *__restrict__ istd, const float *__restrict__ bias, int M, int N,
                   int training, float *__restrict__ dz, float *__restrict__ dnw, float *__restrict__ dnb,
                   float *__restrict__ db, int phase, double *__restrict__ glob, double *__restrict__ local) {
    // phase 0: sums and dz in one pass (every block holds all rows of its columns).  SyncBN cuts it in two around the exchange
    // of the sums over the ranks: phase 1 writes this rank's sums (+ row count) to `glob` and `local`, phase 2 applies the
    // summed `glob` (count at glob[2N]) and takes the parameter gradients from `local`.
    __shared__ double red[8][2][32];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int n = blockIdx.x * 32 + cl;
    const bool ok = n < N;
    float sc = 1.f, sh = 0.f, mu = 0.f, is = 1.f;
    if (ok) {
        if (bn) sc = scale[n], sh = shift[n], mu = mean[n], is = istd[n];
        else sh = bias[n];
    }
    double s1 = 0.0, s2 = 0.0;
    if (ok)
        for (int m = rl; m < M; m += 8) {
            const size_t i = (size_t)m * N + n;
            const float zz = z[i];
            float g = dy[i];
            if (mask) g = mask[i] ? g * drop_scale : 0.f;
            if (relu && !(fmaf(zz, sc, sh) > 0.f)) g = 0.f;
            s1 += (double)g;
            s2 += (double)g * (double)((zz - mu) * is);
        }
    red[rl][0][cl] = s1;
    red[rl][1][cl] = s2;
    __syncthreads();
    s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s1 += red[i][0][cl], s2 += red[i][1][cl];
    if (phase == 1) {
        if (ok && rl == 0) glob[n] = local[n] = s1, glob[N + n] = local[N + n] = s2;
        if (blockIdx.x == 0 && threadIdx.x == 0) glob[2 * N] = local[2 * N] = (double)M;
        return;
    }
    if (!ok) return;
    double count = (double)M;
    if (phase == 2) s1 = glob[n], s2 = glob[N + n], count = glob[2 * N];
    const float c1 = (bn && training) ? (float)(s1 / count) : 0.f, c2 = (bn && training) ? (float)(s2 / count) : 0.f;
    if (phase == 2) s1 = local[n], s2 = local[N + n];
    for (int m = rl; m < M; m += 8) {
        const size_t i = (size_t)m * N + n;
        const float zz = z[i];
        float g = dy[i];
        if (mask) g = mask[i] ? g * drop_scale : 0.f;
        if (relu && !(fmaf(zz, sc, sh) > 0.f)) g = 0.f;
        dz[i] = bn ? sc * (g - c1 - (zz - mu) * is * c2) : g;
    }
    if (rl == 0) {
        if (bn) {
            if (dnw) dnw[n] = (float)s2;
            if (dnb) dnb[n] = (float)s1;
            if (db) db[n] = training ? 0.f : (float)((double)sc * s1);
        } else if (db) {
            db[n] = (float)s1;
        }
    }
}

// ---- backward, BatchNorm1d over many rows (the per-point layers of models/pointnet.py, M = B * N) ------------------------------
// The same arithmetic as fc_bwd_cols_kernel (phase 0) with the rows split over workgroups: 256-row chunks write float64 partial
// sums [chunk][2N] (sum g, sum g * xhat), the apply pass adds them up in chunk order (deterministic) and writes dz and the
// normalisation's parameter gradients.  grid = (N / 64 column blocks, M / 256 row chunks).
__global__ void __launch_bounds__(256)
fc_bwd_bn_rows_sums_kernel(const float *__restrict__ dy, const float *__restrict__ z, const uint8_t *__restrict__ mask,
                           float drop_scale, int relu, const float *__restrict__ scale, const float *__restrict__ shift,
                           const float *__restrict__ mean, const float *__restrict__ istd, int M, int N, double *__restrict__ part) {
    __shared__ double red[4][2][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + cl, m0 = blockIdx.y * 256;
    double s1 = 0.0, s2 = 0.0;
    if (n < N) {
        const float sc = scale[n], sh = shift[n], mu = mean[n], is = istd[n];
        for (int r = rl; r < 256; r += 4) {
            const int m = m0 + r;
            if (m >= M) break;
            const size_t i = (size_t)m * N + n;
            const float zz = z[i];
            float g = dy[i];
            if (mask) g = mask[i] ? g * drop_scale : 0.f;
            if (relu && !(fmaf(zz, sc, sh) > 0.f)) g = 0.f;
            s1 += (double)g;
            s2 += (double)g * (double)((zz - mu) * is);
        }
    }
    red[rl][0][cl] = s1;
    red[rl][1][cl] = s2;
    __syncthreads();
    if (rl == 0 && n < N) {
        part[(size_t)blockIdx.y * 2 * N + n] = (red[0][0][cl] + red[1][0][cl]) + (red[2][0][cl] + red[3][0][cl]);
        part[(size_t)blockIdx.y * 2 * N + N + n] = (red[0][1][cl] + red[1][1][cl]) + (red[2][1][cl] + red[3][1][cl]);
    }
}

__global__ void __launch_bounds__(256)
fc_bwd_bn_rows_apply_kernel(const float *__restrict__ dy, const float *__restrict__ z, const uint8_t *__restrict__ mask,
                            float drop_scale, int relu, const float *__restrict__ scale, const float *__restrict__ shift,
                            const float *__restrict__ mean, const float *__restrict__ istd, int M, int N, int training, int chunks,
                            const double *__restrict__ part, float *__restrict__ dz, float *__restrict__ dnw,
                            float *__restrict__ dnb, float *__restrict__ db) {
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + cl, m0 = blockIdx.y * 256;
    if (n >= N) return;
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < chunks; ++c) s1 += part[(size_t)c * 2 * N + n], s2 += part[(size_t)c * 2 * N + N + n];
    const float sc = scale[n], sh = shift[n], mu = mean[n], is = istd[n];
    const float c1 = training ? (float)(s1 / M) : 0.f, c2 = training ? (float)(s2 / M) : 0.f;
    for (int r = rl; r < 256; r += 4) {
        const int m = m0 + r;
        if (m >= M) break;
        const size_t i = (size_t)m * N + n;
        const float zz = z[i];
        float g = dy[i];
        if (mask) g = mask[i] ? g * drop_scale : 0.f;
        if (relu && !(fmaf(zz, sc, sh) > 0.f)) g = 0.f;
        dz[i] = sc * (g - c1 - (zz - mu) * is * c2);
    }
    if (blockIdx.y == 0 && rl == 0) {
        if (dnw) dnw[n] = (float)s2;
        if (dnb) dnb[n] = (float)s1;
        if (db) db[n] = training ? 0.f : (float)((double)sc * s1);
    }
}

// ---- backward of a head block with at most 32 rows, ONE launch (round 3) ------------------------------------------------------------
// Linear -> BatchNorm1d (or none) -> ReLU -> Dropout, M <= 32 (models/pointnet_pp_vonMises.py:32-35 at batch 32): fc_bwd_cols_kernel
// (dz and the normalisation's parameter gradients, 5 us) and fc_dx_dw_kernel (dx = dz W, dW = dz^T x, 6 - 7 us) only differ by WHO holds
// dz -- and with 32 rows every workgroup that needs a column of dz can hold all of it: the column sums of BatchNorm-backward are sums
// over the rows of ONE tile.  So dz is never written: the dW workgroups (32 columns n x 128 columns k) rebuild their 32 x 32 tile of it
// from dy, z and the keep-mask, the dx workgroups (32 columns k, the reduction over n split over 16 waves) first rebuild ALL of dz --
// 1024 / N threads per column, each with its share of the 32 rows in registers: three coalesced, L2-resident streams -- into an LDS image
// that feeds their MFMA A operand.  (A first version formed the operand while loading it, lane = row: a 2 KB stride between the lanes of
// every load, 26 - 30 us.)  The parameter gradients of the normalisation come from the dW workgroups of the first k block.
// 5.0 + 5.6 and 5.7 + 7.5 us in four launches -> 9.5 and 11.1 us in two.
#ifndef FCF_EXP   // timing experiments (wrong results): 1 no constants pass in the dx tiles, 2 no reduction loop there, 4 no column pass in the dW blocks
#define FCF_EXP 0
#endif
struct FcFusedArgs {
    const float *dy, *z;
    const uint8_t *mask;
    float drop_scale;
    int relu, bn, training;
    const float *scale, *shift, *mean, *istd, *bias;
    const float *w, *x;
    int M, N, K;
    float *dx, *dw, *dnw, *dnb, *db;
    int g1, gx2;
};

__device__ __forceinline__ float fc_masked_g(const FcFusedArgs &P, size_t i, float zz, float sc, float sh) {
    float g = P.dy[i];
    if (P.mask) g = P.mask[i] ? g * P.drop_scale : 0.f;
    if (P.relu && !(fmaf(zz, sc, sh) > 0.f)) g = 0.f;
    return g;
}

template <int TPC>   // threads per column of dz in the dx tiles' first pass (1024 / TPC columns at a time, 32 / TPC rows per thread)
__global__ void __launch_bounds__(1024) fc_bwd_fused_kernel(const FcFusedArgs P) {
    extern __shared__ __attribute__((aligned(16))) float fl[];
    const int tid = threadIdx.x, M = P.M, N = P.N, K = P.K;
    if ((int)blockIdx.x >= P.g1) {
        // ---- dW block: columns n0 .. n0 + 32 of dz (all rows), columns k0 .. k0 + 128 of x ----
        float (*dzs)[32] = reinterpret_cast<float (*)[32]>(fl);                    // [32][32]
        float (*xs)[128] = reinterpret_cast<float (*)[128]>(fl + 32 * 32);         // [32][128]
        float (*gs)[32] = reinterpret_cast<float (*)[32]>(fl + 32 * 32 + 32 * 128);   // masked upstream gradient
        float (*zs)[32] = gs + 32;                                                  // xhat (bn) of the same elements
        const int bx = ((int)blockIdx.x - P.g1) % P.gx2, by = ((int)blockIdx.x - P.g1) / P.gx2;
        const int k0 = bx * 128, n0 = by * 32;
        {
            const int m = tid >> 5, n = tid & 31, nn = n0 + n;
            float g = 0.f, xh = 0.f;
            if (m < M && nn < N) {
                const size_t i = (size_t)m * N + nn;
                const float zz = P.z[i];
                const float sc = P.bn ? P.scale[nn] : 1.f, sh = P.bn ? P.shift[nn] : P.bias[nn];
                g = fc_masked_g(P, i, zz, sc, sh);
                if (P.bn) xh = (zz - P.mean[nn]) * P.istd[nn];
            }
            gs[m][n] = g, zs[m][n] = xh;
        }
        for (int f = tid; f < 32 * 128; f += 1024) {
            const int m = f >> 7, k = f & 127;
            xs[m][k] = (m < M && k0 + k < K) ? P.x[(size_t)m * K + k0 + k] : 0.f;
        }
        __syncthreads();
        if (tid < 32 && !(FCF_EXP & 4)) {   // one thread per column: the sums over the rows, in row order
            const int nn = n0 + tid;
            double s1 = 0.0, s2 = 0.0;
            for (int m = 0; m < 32; ++m) s1 += (double)gs[m][tid], s2 += (double)gs[m][tid] * (double)zs[m][tid];
            const float sc = (P.bn && nn < N) ? P.scale[nn] : 1.f;
            const float c1 = (P.bn && P.training) ? (float)(s1 / (double)M) : 0.f, c2 = (P.bn && P.training) ? (float)(s2 / (double)M) : 0.f;
            for (int m = 0; m < 32; ++m) dzs[m][tid] = (m < M && nn < N) ? (P.bn ? sc * (gs[m][tid] - c1 - zs[m][tid] * c2) : gs[m][tid]) : 0.f;
            if (bx == 0 && nn < N) {
                if (P.bn) {
                    if (P.dnw) P.dnw[nn] = (float)s2;
                    if (P.dnb) P.dnb[nn] = (float)s1;
                    // a bias in front of a train-mode BatchNorm has exactly zero gradient; with running statistics d(bias) = scale sum g
                    if (P.db) P.db[nn] = P.training ? 0.f : (float)((double)sc * s1);
                } else if (P.db) {
                    P.db[nn] = (float)s1;
                }
            }
        }
        __syncthreads();
        const int kl = tid & 127, nh = tid >> 7;
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
                if (n < N) P.dw[(size_t)n * K + k0 + kl] = acc[j];
            }
        return;
    }
    // ---- dx tile: columns k0 .. k0 + 32 of dx = dz W.  Pass 1: thread n holds column n of all 32 rows (three coalesced streams,
    // eight rows in flight at a time), sums it, and writes its dz column to an LDS image [32][N + 1]; pass 2: wave w takes the
    // reduction indices n = 2 w + 32 j (+ lane half) from that image, W from global memory (coalesced over the 32 output columns) ----
    const int DP = N + 1;
    float *dzs = fl;                                 // [32][N + 1]; afterwards [16 waves][16 registers][64 lanes] partial tiles
    const int k0 = (int)blockIdx.x * 32;
    const int lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const bool colok = k0 + l31 < K;
    const float *wcol = P.w + k0 + (colok ? l31 : 0);
    constexpr int CPP = 1024 / TPC, R = 32 / TPC;    // columns per pass, rows per thread
    double *ps = reinterpret_cast<double *>(fl + ((32 * DP + 1) & ~1));   // [TPC][2][CPP] partial sums of a pass
    for (int c0 = 0; c0 < ((FCF_EXP & 1) ? 0 : N); c0 += CPP) {
        const int cl = tid % CPP, rg = tid / CPP, n = c0 + cl, nc = min(n, N - 1);
        const float sc = P.bn ? P.scale[nc] : 1.f, sh = P.bn ? P.shift[nc] : P.bias[nc];
        const float mu = P.bn ? P.mean[nc] : 0.f, is = P.bn ? P.istd[nc] : 0.f;
        float g[R], xh[R];
#pragma unroll
        for (int m0 = 0; m0 < R; m0 += 8) {
            float zr[8], gr[8];
            unsigned char kr[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned i = (unsigned)min(rg * R + m0 + j, M - 1) * (unsigned)N + (unsigned)nc;
                zr[j] = P.z[i], gr[j] = P.dy[i], kr[j] = P.mask ? P.mask[i] : (unsigned char)1;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float gg = kr[j] ? gr[j] * (P.mask ? P.drop_scale : 1.f) : 0.f;
                if (P.relu && !(fmaf(zr[j], sc, sh) > 0.f)) gg = 0.f;
                if (rg * R + m0 + j >= M) gg = 0.f;
                g[m0 + j] = gg, xh[m0 + j] = (zr[j] - mu) * is;
            }
        }
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int m = 0; m < R; ++m) s1 += (double)g[m], s2 += (double)g[m] * (double)xh[m];
        if (TPC > 1) {   // the row groups of a column, in row order
            ps[(rg * 2 + 0) * CPP + cl] = s1, ps[(rg * 2 + 1) * CPP + cl] = s2;
            __syncthreads();
            s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int q = 0; q < TPC; ++q) s1 += ps[(q * 2 + 0) * CPP + cl], s2 += ps[(q * 2 + 1) * CPP + cl];
            __syncthreads();
        }
        const float c1 = (P.bn && P.training) ? (float)(s1 / (double)M) : 0.f, c2 = (P.bn && P.training) ? (float)(s2 / (double)M) : 0.f;
        if (n < N)
#pragma unroll
            for (int m = 0; m < R; ++m) dzs[(rg * R + m) * DP + n] = rg * R + m < M ? (P.bn ? sc * (g[m] - c1 - xh[m] * c2) : g[m]) : 0.f;
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *arow = dzs + l31 * DP + lh;
    // (all sixteen steps' weights requested at the top of the kernel, ahead of pass 1: 11.1 -> 15.0 us -- sixteen more live registers
    // spill at the 128 a 1,024-thread workgroup leaves a lane)
    for (int nb0 = 2 * wave; nb0 < ((FCF_EXP & 2) ? 0 : N); nb0 += 32 * 8) {   // eight steps' weights requested together
        float wr[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) wr[j] = wcol[(size_t)min(nb0 + 32 * j + lh, N - 1) * K];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = nb0 + 32 * j + lh;
            const float a = n < N ? arow[min(nb0 + 32 * j, N - 2)] : 0.f, b = (colok && n < N) ? wr[j] : 0.f;
            if (nb0 + 32 * j < N) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);   // (uniform)
        }
    }
    __syncthreads();   // every wave is done with the image: the partial tiles take its place
    float *red = fl;
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    {   // one thread per output element: the sixteen partial tiles in wave order
        const int r = tid >> 6, ln = tid & 63;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += red[(w * 16 + r) * 64 + ln];
        const int row = (r & 3) + 4 * (ln >> 5) + 8 * (r >> 2), col = k0 + (ln & 31);
        if (row < M && col < K) P.dx[(size_t)row * K + col] = t;
    }
}

// ---- backward, LayerNorm: one block per row writes dz and g; column sums in a second kernel ---------
__global__ void __launch_bounds__(256)
fc_bwd_ln_rows_kernel(const float *__restrict__ dy, const float *__restrict__ z, const float *__restrict__ b,
                      const float *__restrict__ nw, const float *__restrict__ nb, const uint8_t *__restrict__ mask,
                      float drop_scale, int relu, const float *__restrict__ mean, const float *__restrict__ istd, int N,
                      float *__restrict__ dz, float *__restrict__ gbuf) {
    __shared__ double red[2][4];
    const int m = blockIdx.x;
    const float mu = mean[m], is = istd[m];
    double s1 = 0.0, s2 = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const size_t i = (size_t)m * N + n;
        const float xh = ((z[i] + b[n]) - mu) * is;
        float g = dy[i];
        if (mask) g = mask[i] ? g * drop_scale : 0.f;
        if (relu && !(xh * nw[n] + nb[n] > 0.f)) g = 0.f;
        gbuf[i] = g;
        const double gh = (double)g * (double)nw[n];
        s1 += gh;
        s2 += gh * (double)xh;
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s1 += shfl_xor_f64(s1, k), s2 += shfl_xor_f64(s2, k);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = s1, red[1][threadIdx.x >> 6] = s2;
    __syncthreads();
    const float c1 = (float)(((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / N);
    const float c2 = (float)(((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / N);
    for (int n = threadIdx.x; n < N; n += 256) {
        const size_t i = (size_t)m * N + n;
        const float xh = ((z[i] + b[n]) - mu) * is;
        dz[i] = is * (gbuf[i] * nw[n] - c1 - xh * c2);
    }
}

__global__ void __launch_bounds__(256)
fc_bwd_ln_cols_kernel(const float *__restrict__ gbuf, const float *__restrict__ dz, const float *__restrict__ z,
                      const float *__restrict__ b, const float *__restrict__ mean, const float *__restrict__ istd, int M, int N,
                      float *__restrict__ dnw, float *__restrict__ dnb, float *__restrict__ db) {
    __shared__ double red[8][3][32];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int n = blockIdx.x * 32 + cl;
    double a = 0.0, c = 0.0, e = 0.0;
    if (n < N)
        for (int m = rl; m < M; m += 8) {
            const size_t i = (size_t)m * N + n;
            const float xh = ((z[i] + b[n]) - mean[m]) * istd[m];
            a += (double)gbuf[i] * (double)xh;
            c += (double)gbuf[i];
            e += (double)dz[i];
        }
    red[rl][0][cl] = a, red[rl][1][cl] = c, red[rl][2][cl] = e;
    __syncthreads();
    if (rl == 0 && n < N) {
        a = c = e = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) a += red[i][0][cl], c += red[i][1][cl], e += red[i][2][cl];
        if (dnw) dnw[n] = (float)a;
        if (dnb) dnb[n] = (float)c;
        if (db) db[n] = (float)e;
    }
}

// ---- narrow output layers (N <= 16, no norm): fc3 / head_pi / head_mu / head_kappa ------------------
// Too narrow for a 32-wide MFMA tile; these are K-long dot products, one wavefront per output element.  (FC_SMALL_N: fc.h)
__global__ void __launch_bounds__(256) fc_small_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                           const float *__restrict__ b, const uint8_t *__restrict__ mask,
                                                           float drop_scale, int relu, int K, int N, float *__restrict__ z,
                                                           float *__restrict__ y) {
    const int m = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *xr = x + (size_t)m * K;
    for (int n = wave; n < N; n += 4) {
        const float *wr = w + (size_t)n * K;
        double acc = 0.0;
        for (int k = lane; k < K; k += 64) acc += (double)xr[k] * (double)wr[k];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) acc += shfl_xor_f64(acc, s);
        if (lane == 0) {
            const float zz = (float)acc;  // bias-free pre-activation, like the MFMA path keeps it
            z[(size_t)m * N + n] = zz;
            float v = zz + b[n];
            if (relu) v = fmaxf(v, 0.f);
            if (mask) v = mask[(size_t)m * N + n] ? v * drop_scale : 0.f;
            y[(size_t)m * N + n] = v;
        }
    }
}

__device__ __forceinline__ float fc_small_dz(const float *dy, const float *z, const float *b, const uint8_t *mask,
                                             float drop_scale, int relu, size_t i, int n) {
    float g = dy[i];
    if (mask) g = mask[i] ? g * drop_scale : 0.f;
    if (relu && !(z[i] + b[n] > 0.f)) g = 0.f;
    return g;
}

// One launch for the whole backward of a narrow layer.  Workgroups [0, N * kparts): dW[n][k] = sum_m dz[m][n] x[m][k]
// for one n and one 256-wide k range (the first range of every n also writes db[n] = sum_m dz[m][n]); the dz column
// is staged in LDS once, so the m loop is independent loads.  Workgroups after those: dx[m][:] = sum_n dz[m][n] w[n][:].
__global__ void __launch_bounds__(256) fc_small_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ z,
                                                           const float *__restrict__ b, const uint8_t *__restrict__ mask,
                                                           float drop_scale, int relu, const float *__restrict__ x,
                                                           const float *__restrict__ w, int M, int K, int N, int kparts,
                                                           float *__restrict__ dw, float *__restrict__ db,
                                                           float *__restrict__ dx) {
    __shared__ float dzc[1024];
    const int ndw = N * kparts;
    if ((int)blockIdx.x < ndw) {
        const int n = blockIdx.x / kparts, k = (blockIdx.x % kparts) * 256 + threadIdx.x;
        double acc = 0.0, accb = 0.0;
        for (int m0 = 0; m0 < M; m0 += 1024) {  // M rows in LDS-sized pieces (a training batch is one piece)
            const int mc = min(1024, M - m0);
            __syncthreads();
            for (int m = threadIdx.x; m < mc; m += 256)
                dzc[m] = fc_small_dz(dy, z, b, mask, drop_scale, relu, (size_t)(m0 + m) * N + n, n);
            __syncthreads();
            if (k < K) {
                const float *xc = x + (size_t)m0 * K + k;
#pragma unroll 8
                for (int m = 0; m < mc; ++m) acc += (double)dzc[m] * (double)xc[(size_t)m * K];
            }
            if (threadIdx.x == 0 && blockIdx.x % kparts == 0)
                for (int m = 0; m < mc; ++m) accb += (double)dzc[m];
        }
        if (k < K) dw[(size_t)n * K + k] = (float)acc;
        if (threadIdx.x == 0 && blockIdx.x % kparts == 0) db[n] = (float)accb;
        return;
    }
    if (!dx) return;
    const int m = blockIdx.x - ndw;
    float g[FC_SMALL_N];
#pragma unroll
    for (int n = 0; n < FC_SMALL_N; ++n)
        g[n] = fc_small_dz(dy, z, b, mask, drop_scale, relu, (size_t)m * N + min(n, N - 1), min(n, N - 1)) * (n < N ? 1.f : 0.f);
    for (int k = threadIdx.x; k < K; k += 256) {
        float acc = 0.f;
#pragma unroll
        for (int n = 0; n < FC_SMALL_N; ++n)
            if (n < N) acc = fmaf(g[n], w[(size_t)n * K + k], acc);
        dx[(size_t)m * K + k] = acc;
    }
}

// dW (N,K) = dz^T x for a batch of at most 32 rows (the head layers): an outer-product accumulation with no reduction
// worth an MFMA tile.  Workgroup = 32 output rows (n) x 128 output columns (k): dz tile and x tile in LDS, each thread
// owns one k and sixteen n.  Stores are 512-byte rows.
__global__ void __launch_bounds__(256) dw_fewrows_kernel(const float *__restrict__ dz, const float *__restrict__ x, int M, int N,
                                                         int K, float *__restrict__ dw) {
    __shared__ __attribute__((aligned(16))) float dzs[32][32];
    __shared__ float xs[32][128];
    const int kl = threadIdx.x & 127, nh = threadIdx.x >> 7;
    const int k0 = blockIdx.x * 128, n0 = blockIdx.y * 32;
    for (int f = threadIdx.x; f < 32 * 32; f += 256) {
        const int m = f >> 5, n = f & 31;
        dzs[m][n] = (m < M && n0 + n < N) ? dz[(size_t)m * N + n0 + n] : 0.f;
    }
    for (int f = threadIdx.x; f < 32 * 128; f += 256) {
        const int m = f >> 7, k = f & 127;
        xs[m][k] = (m < M && k0 + k < K) ? x[(size_t)m * K + k0 + k] : 0.f;
    }
    __syncthreads();
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
#pragma unroll 4
    for (int m = 0; m < 32; ++m) {
        const float xv = xs[m][kl];
        const float4 *d4 = reinterpret_cast<const float4 *>(&dzs[m][16 * nh]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 d = d4[q];
            acc[4 * q] = fmaf(d.x, xv, acc[4 * q]), acc[4 * q + 1] = fmaf(d.y, xv, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(d.z, xv, acc[4 * q + 2]), acc[4 * q + 3] = fmaf(d.w, xv, acc[4 * q + 3]);
        }
    }
    if (k0 + kl < K)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int n = n0 + 16 * nh + j;
            if (n < N) dw[(size_t)n * K + k0 + kl] = acc[j];
        }
}

// ---- launchers (fc.h): one per kernel; each hands its kernel the argument values the call sites used to spell out -----------------
int launch_fc_apply_cols(const float *z, const float *scale, const float *shift, const uint8_t *mask, float drop_scale, int relu, int M,
                         int N, float *y, bool tagged, const char *what, hipStream_t st) {
    const size_t total = (size_t)M * N;
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    auto go = [&] { hipLaunchKernelGGL(fc_apply_cols_kernel, dim3(grid), dim3(256), 0, st, z, scale, shift, mask, drop_scale, relu, M, N, y); };
    if (tagged) {
        ProfScope ps(st, "fc_apply_cols_kernel M=%d N=%d", M, N);
        go();
    } else {
        go();
    }
    PNPP_CHECK_LAUNCH(what);
    return PNPP_OK;
}

int launch_fc_apply_ln(const float *z, const float *b, const float *nw, const float *nb, const uint8_t *mask, float drop_scale, int relu,
                       int M, int N, float eps, float *y, float *mean, float *istd, const FcDraw &draw, hipStream_t st) {
    hipLaunchKernelGGL(fc_apply_ln_kernel, dim3(M), dim3(256), 0, st, z, b, nw, nb, mask, drop_scale, relu, N, eps, y, mean, istd,
                       draw.mask_out, draw.drop_p, draw.rng_seed, draw.rng_counter);
    PNPP_CHECK_LAUNCH("fc_forward");
    return PNPP_OK;
}

int launch_fc_bwd_rows(const FcGrad &g, float *dz, float *slab, hipStream_t st) {
    ProfScope ps(st, "fc_bwd_rows_kernel M=%d N=%d", g.M, g.N);
    hipLaunchKernelGGL(fc_bwd_rows_kernel, dim3(cdiv(g.N, 64), fc_row_chunks(g.M)), dim3(256), 0, st, g.dy, g.z, g.mask, g.drop_scale,
                       g.relu, g.bias, g.M, g.N, dz, slab);
    PNPP_CHECK_LAUNCH("fc_backward(rows)");
    return PNPP_OK;
}

int launch_fc_bwd_cols(const FcGrad &g, float *dz, const BnGrads &pg, int phase, double *glob, double *local, hipStream_t st) {
    hipLaunchKernelGGL(fc_bwd_cols_kernel, dim3(cdiv(g.N, 32)), dim3(256), 0, st, g.dy, g.z, g.mask, g.drop_scale, g.relu, g.bn, g.scale,
                       g.shift, g.mean, g.istd, g.bias, g.M, g.N, g.training, dz, pg.dgamma, pg.dbeta, pg.dbias, phase, glob, local);
    PNPP_CHECK_LAUNCH(phase == 1 ? "fc_backward(sums)" : "fc_backward");
    return PNPP_OK;
}

int launch_fc_bwd_bn_rows_sums(const FcGrad &g, double *part, hipStream_t st) {
    ProfScope ps(st, "fc_bwd_bn_rows_sums_kernel M=%d N=%d", g.M, g.N);
    hipLaunchKernelGGL(fc_bwd_bn_rows_sums_kernel, dim3(cdiv(g.N, 64), fc_row_chunks(g.M)), dim3(256), 0, st, g.dy, g.z, g.mask,
                       g.drop_scale, g.relu, g.scale, g.shift, g.mean, g.istd, g.M, g.N, part);
    PNPP_CHECK_LAUNCH("fc_backward(bn sums)");
    return PNPP_OK;
}

int launch_fc_bwd_bn_rows_apply(const FcGrad &g, const double *part, float *dz, const BnGrads &pg, hipStream_t st) {
    const int chunks = fc_row_chunks(g.M);
    ProfScope ps(st, "fc_bwd_bn_rows_apply_kernel M=%d N=%d", g.M, g.N);
    hipLaunchKernelGGL(fc_bwd_bn_rows_apply_kernel, dim3(cdiv(g.N, 64), chunks), dim3(256), 0, st, g.dy, g.z, g.mask, g.drop_scale, g.relu,
                       g.scale, g.shift, g.mean, g.istd, g.M, g.N, g.training, chunks, part, dz, pg.dgamma, pg.dbeta, pg.dbias);
    PNPP_CHECK_LAUNCH("fc_backward");
    return PNPP_OK;
}

int launch_fc_bwd_ln_rows(const FcGrad &g, const float *nw, const float *nb, float *dz, float *gbuf, hipStream_t st) {
    hipLaunchKernelGGL(fc_bwd_ln_rows_kernel, dim3(g.M), dim3(256), 0, st, g.dy, g.z, g.bias, nw, nb, g.mask, g.drop_scale, g.relu, g.mean,
                       g.istd, g.N, dz, gbuf);
    PNPP_CHECK_LAUNCH("fc_backward");
    return PNPP_OK;
}

int launch_fc_bwd_ln_cols(const FcGrad &g, const float *gbuf, const float *dz, const BnGrads &pg, hipStream_t st) {
    hipLaunchKernelGGL(fc_bwd_ln_cols_kernel, dim3(cdiv(g.N, 32)), dim3(256), 0, st, gbuf, dz, g.z, g.bias, g.mean, g.istd, g.M, g.N,
                       pg.dgamma, pg.dbeta, pg.dbias);
    PNPP_CHECK_LAUNCH("fc_backward");
    return PNPP_OK;
}

static int fc_fused_tpc(int N) { return N <= 256 ? 4 : N <= 512 ? 2 : 1; }
size_t fc_bwd_fused_lds(int N) {
    const int tpc = fc_fused_tpc(N);
    const size_t img = (size_t)32 * (N + 1) + 2 + (size_t)tpc * 2 * (1024 / tpc) * 2, part = (size_t)16 * 16 * 64;
    const size_t lds_dx = (img > part ? img : part) * sizeof(float), lds_dw = (size_t)(32 * 32 + 32 * 128 + 2 * 32 * 32) * sizeof(float);
    return lds_dx > lds_dw ? lds_dx : lds_dw;
}

int launch_fc_bwd_fused(const FcGrad &g, const float *w, const float *x, int K, float *dx, float *dw, const BnGrads &pg, hipStream_t st) {
    FcFusedArgs P;
    P.dy = g.dy, P.z = g.z, P.mask = g.mask, P.drop_scale = g.drop_scale, P.relu = g.relu, P.bn = g.bn, P.training = g.training;
    P.scale = g.scale, P.shift = g.shift, P.mean = g.mean, P.istd = g.istd, P.bias = g.bias;
    P.w = w, P.x = x, P.M = g.M, P.N = g.N, P.K = K;
    P.dx = dx, P.dw = dw, P.dnw = pg.dgamma, P.dnb = pg.dbeta, P.db = pg.dbias;
    P.g1 = cdiv(K, 32), P.gx2 = cdiv(K, 128);
    const int gy2 = cdiv(g.N, 32);
    const int tpc = fc_fused_tpc(g.N);
    const size_t lds = fc_bwd_fused_lds(g.N);
    auto go = [&](auto tc) {
        constexpr auto kfn = fc_bwd_fused_kernel<tc()>;
        grant_lds<kfn>(lds);
        hipLaunchKernelGGL(kfn, dim3(P.g1 + P.gx2 * gy2), dim3(1024), lds, st, P);
    };
    ProfScope ps(st, "fc_bwd_fused_kernel M=%d N=%d K=%d grid=%d+%d", g.M, g.N, K, P.g1, P.gx2 * gy2);
    if (tpc == 4) go(mode_c<4>{});
    else if (tpc == 2) go(mode_c<2>{});
    else go(mode_c<1>{});
    PNPP_CHECK_LAUNCH("fc_backward(fused)");
    return PNPP_OK;
}

int launch_fc_small_fwd(const float *x, const float *w, const float *b, const uint8_t *mask, float drop_scale, int relu, int M, int K, int N,
                        float *z, float *y, hipStream_t st) {
    ProfScope ps(st, "fc_small_fwd_kernel M=%d N=%d K=%d", M, N, K);
    hipLaunchKernelGGL(fc_small_fwd_kernel, dim3(M), dim3(256), 0, st, x, w, b, mask, drop_scale, relu, K, N, z, y);
    PNPP_CHECK_LAUNCH("fc_forward(small)");
    return PNPP_OK;
}

int launch_fc_small_bwd(const FcGrad &g, const float *x, const float *w, int K, float *dw, float *db, float *dx, hipStream_t st) {
    ProfScope ps(st, "fc_small_bwd M=%d N=%d K=%d", g.M, g.N, K);
    const int kparts = cdiv(K, 256);
    hipLaunchKernelGGL(fc_small_bwd_kernel, dim3(g.N * kparts + (dx ? g.M : 0)), dim3(256), 0, st, g.dy, g.z, g.bias, g.mask, g.drop_scale,
                       g.relu, x, w, g.M, K, g.N, kparts, dw, db, dx);
    PNPP_CHECK_LAUNCH("fc_backward(small)");
    return PNPP_OK;
}

int launch_dw_fewrows(const float *dz, const float *x, int M, int N, int K, float *dw, hipStream_t st) {
    ProfScope ps(st, "dw_fewrows_kernel M=%d N=%d K=%d", M, N, K);
    hipLaunchKernelGGL(dw_fewrows_kernel, dim3(cdiv(K, 128), cdiv(N, 32)), dim3(256), 0, st, dz, x, M, N, K, dw);
    PNPP_CHECK_LAUNCH("fc_backward(dw)");
    return PNPP_OK;
}

unsigned fc_build_flags() { return (FCF_EXP != 0) ? 32u : 0u; }

}  // namespace pnpp
