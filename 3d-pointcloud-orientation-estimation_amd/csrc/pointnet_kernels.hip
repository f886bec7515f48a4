// pointnet_kernels.hip -- kernels of the vanilla PointNet (models/pointnet.py): the pooled wide layer, the per-cloud transforms,
// the feature-transform regulariser and the small pieces of the heads.  All products are float32 (statistics and reductions over
// points in float64); the process-wide product switches of the set-abstraction path (pnpp_set_matmul_precision /
// pnpp_set_split_products) do not apply here.
//
// The pooled wide layer ("Vanilla PointNet"): z = A W^T + b, y = act(a_c (z - mu_c) + beta_c) with a_c = gamma_c istd_c,
// pooled = max_n y.  BatchNorm is a per-channel monotone affine map and ReLU is monotone, so the pooled value is act(a_c (zsel - mu_c)
// + beta_c) with zsel the cloud's max of z where a_c >= 0 and its min otherwise.  The forward pass keeps per (cloud, channel) the max /
// min of z and their rows only; the training statistics come from the column sums S and the Gram matrix G of A; the backward pass
// is one M x K x K product with Q = W^T diag(a m istd) W plus a routed scatter.
//
// Ragged batches ("Vanilla PointNet", "Ragged batches"): the kernels that address rows per cloud carry a RAGGED template
// flag.  The valid rows are packed once, by pn_transform_kernel<true>, and addressed through the lengths' prefix sum `offs`; the
// <false> instantiations are the uniform kernels as they were.
#include "pointnet.h"

#include <math.h>

namespace pnpp {

constexpr int PN_KMAX = 128;   // input width of the pooled layer (the three trunks: 128)
constexpr int PN_CB = 64;      // channels per workgroup of the max / min scan
constexpr int PN_RT = 64;      // rows per tile
constexpr int PN_CMAX = 1024;  // channels of the pooled layer (routed-scatter lists in LDS)
constexpr int PN_TMAX = 64;    // largest transform

__device__ inline double wave_sum_to0(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;  // complete in lane 0 only
}
__device__ inline double wave_sum(double v) { return __shfl(wave_sum_to0(v), 0, 64); }

// Ragged batches (RAGGED kernels): the clouds' valid rows are packed one cloud after the other, offs (B + 1) int32 their exclusive
// prefix sum -- row n of cloud b at offs[b] + n, Nv = offs[b + 1] - offs[b] of the padded N.  b is a block index, so the two loads
// are wave-uniform.  Uniform batches: row b * N + n, Nv = N.
template <bool RAGGED>
__device__ __forceinline__ void pn_cloud_rows(const int32_t *__restrict__ offs, int b, int N, size_t &row0, int &Nv) {
    if (RAGGED) {
        const int o0 = offs[b], o1 = offs[b + 1];
        row0 = (size_t)o0;
        Nv = min(max(o1 - o0, 0), N);
    } else {
        row0 = (size_t)b * N;
        Nv = N;
    }
}

// lens_out[b] = min(max(lengths[b], 1), N) and offs = their exclusive prefix sum (B + 1 entries): one workgroup, every thread a
// run of consecutive clouds, the 256 run totals scanned by thread 0
__global__ void __launch_bounds__(256) pn_offsets_kernel(const int32_t *__restrict__ lengths, int B, int N, int32_t *__restrict__ lens_out,
                                                         int32_t *__restrict__ offs) {
    __shared__ int run[256];
    const int t = threadIdx.x, per = (B + 255) / 256, b0 = min(t * per, B), b1 = min(b0 + per, B);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += min(max(lengths[b], 1), N);
    run[t] = s;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int i = 0; i < 256; ++i) {
            const int x = run[i];
            run[i] = acc;
            acc += x;
        }
        offs[B] = acc;
    }
    __syncthreads();
    int acc = run[t];
    for (int b = b0; b < b1; ++b) {
        const int n = min(max(lengths[b], 1), N);
        lens_out[b] = n;
        offs[b] = acc;
        acc += n;
    }
}

int launch_pn_offsets(const int32_t *lengths, int B, int N, int32_t *lens_out, int32_t *offs, hipStream_t st) {
    ProfScope ps(st, "pn_offsets_kernel B=%d", B);
    hipLaunchKernelGGL(pn_offsets_kernel, dim3(1), dim3(256), 0, st, lengths, B, N, lens_out, offs);
    PNPP_CHECK_LAUNCH("pn_offsets");
    return PNPP_OK;
}

// ------------------------------------------------------------------------------------------------
// train-mode statistics: per-cloud Gram matrix / column sums (float64), then their sums and the centred Gram matrix
// ------------------------------------------------------------------------------------------------
// RAGGED: the slices are those of the padded N, so lengths == N gives the uniform reduction order; a (cloud, slice) without a valid
// row writes zero partials
template <bool RAGGED>
__global__ void __launch_bounds__(256) pn_gram_kernel(const float *__restrict__ a, const int32_t *__restrict__ offs, int N, int K,
                                                       int rows_per_slice, double *__restrict__ gp, double *__restrict__ sp) {
    __shared__ float As[32][PN_KMAX];
    const int nt = (K + 63) / 64;
    const int ti = blockIdx.x / nt, tj = blockIdx.x % nt, b = blockIdx.y, t = threadIdx.x;
    const int slice = blockIdx.z, part = b * gridDim.z + slice;   // partials in (cloud, slice) order
    size_t row0;
    int Nv;
    pn_cloud_rows<RAGGED>(offs, b, N, row0, Nv);
    const int nbeg = slice * rows_per_slice, nend = min(Nv, nbeg + rows_per_slice);
    const int li = ti * 64 + (t / 16) * 4, lj = tj * 64 + (t % 16) * 4;
    double acc[4][4] = {};
    double s = 0.0;
    const bool diag = ti == tj && t < 64;
    const int scol = ti * 64 + t;
    for (int n0 = nbeg; n0 < nend; n0 += 32) {
        __syncthreads();
        for (int idx = t; idx < 32 * PN_KMAX; idx += 256) {
            const int r = idx / PN_KMAX, k = idx % PN_KMAX, n = n0 + r;
            As[r][k] = (n < nend && k < K) ? a[(row0 + n) * K + k] : 0.f;
        }
        __syncthreads();
        for (int r = 0; r < 32; ++r) {
            double av[4], bv[4];
            for (int p = 0; p < 4; ++p) {
                av[p] = As[r][li + p < PN_KMAX ? li + p : 0];
                bv[p] = As[r][lj + p < PN_KMAX ? lj + p : 0];
            }
            for (int p = 0; p < 4; ++p)
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(av[p], bv[q], acc[p][q]);
            if (diag && scol < K) s += As[r][scol];
        }
    }
    for (int p = 0; p < 4; ++p)
        for (int q = 0; q < 4; ++q)
            if (li + p < K && lj + q < K) gp[(size_t)part * K * K + (size_t)(li + p) * K + lj + q] = acc[p][q];
    if (diag && scol < K) sp[(size_t)part * K + scol] = s;
}

__global__ void pn_gram_reduce_kernel(const double *__restrict__ gp, const double *__restrict__ sp, int B, int K, double M,
                                      double *__restrict__ S, double *__restrict__ Cc) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= K * K) return;
    const int i = idx / K, j = idx % K;
    double g = 0.0, si = 0.0, sj = 0.0;
    for (int b = 0; b < B; ++b) {
        g += gp[(size_t)b * K * K + idx];
        si += sp[(size_t)b * K + i];
        sj += sp[(size_t)b * K + j];
    }
    Cc[idx] = g - si * sj / M;
    if (j == 0) S[i] = si;
}

int pn_gram_slices(int N) { return N >= 8 * 128 ? 8 : N >= 4 * 64 ? 4 : 1; }

int launch_pn_gram(const float *a, const int32_t *offs, long long M, int B, int N, int K, double *gp, double *sp, double *S, double *Cc,
                   hipStream_t st) {
    const int nt = cdiv(K, 64), ns = pn_gram_slices(N), rps = cdiv(cdiv(N, ns), 32) * 32;
    {
        ProfScope ps(st, "pn_gram_kernel B=%d N=%d K=%d slices=%d", B, N, K, ns);
        if (offs)
            hipLaunchKernelGGL(pn_gram_kernel<true>, dim3(nt * nt, B, ns), dim3(256), 0, st, a, offs, N, K, rps, gp, sp);
        else
            hipLaunchKernelGGL(pn_gram_kernel<false>, dim3(nt * nt, B, ns), dim3(256), 0, st, a, offs, N, K, rps, gp, sp);
        PNPP_CHECK_LAUNCH("pn_gram");
    }
    ProfScope ps(st, "pn_gram_reduce_kernel K=%d", K);
    hipLaunchKernelGGL(pn_gram_reduce_kernel, dim3(cdiv(K * K, 256)), dim3(256), 0, st, gp, sp, B * ns, K, (double)M, S, Cc);
    PNPP_CHECK_LAUNCH("pn_gram_reduce");
    return PNPP_OK;
}

// ------------------------------------------------------------------------------------------------
// the max / min scan: one workgroup per (64-channel block, cloud) loops over the cloud's rows; z never leaves registers
// ------------------------------------------------------------------------------------------------
template <bool RAGGED>
__global__ void __launch_bounds__(256) pn_pool_scan_kernel(const float *__restrict__ a, const int32_t *__restrict__ offs,
                                                            const float *__restrict__ w, const float *__restrict__ bias, int N, int K, int C,
                                                            float *__restrict__ zmax, int32_t *__restrict__ imax,
                                                            float *__restrict__ zmin, int32_t *__restrict__ imin) {
    __shared__ __attribute__((aligned(16))) float Ws[PN_KMAX][PN_CB];
    __shared__ __attribute__((aligned(16))) float As[PN_KMAX][PN_RT];
    const int c0 = blockIdx.x * PN_CB, b = blockIdx.y, t = threadIdx.x;
    const int tc = t % 16, tr = t / 16;
    const int K4 = K / 4;
    for (int idx = t; idx < PN_CB * K; idx += 256) {
        const int c = idx / K, k = idx % K;
        Ws[k][c] = w[(size_t)(c0 + c) * K + k];
    }
    float bc[4];
    for (int q = 0; q < 4; ++q) bc[q] = bias[c0 + tc * 4 + q];
    float vmax[4], vmin[4];
    int jmax[4], jmin[4];
    for (int q = 0; q < 4; ++q) vmax[q] = -INFINITY, vmin[q] = INFINITY, jmax[q] = 0, jmin[q] = 0;
    size_t row0;
    int Nv;
    pn_cloud_rows<RAGGED>(offs, b, N, row0, Nv);
    const float *ab = a + row0 * K;
    for (int n0 = 0; n0 < Nv; n0 += PN_RT) {
        __syncthreads();
        for (int idx = t; idx < PN_RT * K4; idx += 256) {
            const int r = idx / K4, k4 = idx % K4, n = n0 + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < Nv) v = *reinterpret_cast<const float4 *>(ab + (size_t)n * K + k4 * 4);
            As[k4 * 4 + 0][r] = v.x;
            As[k4 * 4 + 1][r] = v.y;
            As[k4 * 4 + 2][r] = v.z;
            As[k4 * 4 + 3][r] = v.w;
        }
        __syncthreads();
        float acc[4][4] = {};
        for (int k = 0; k < K; ++k) {
            const float4 av = *reinterpret_cast<const float4 *>(&As[k][tr * 4]);
            const float4 wv = *reinterpret_cast<const float4 *>(&Ws[k][tc * 4]);
            const float ar[4] = {av.x, av.y, av.z, av.w}, wr[4] = {wv.x, wv.y, wv.z, wv.w};
            for (int p = 0; p < 4; ++p)
                for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(ar[p], wr[q], acc[p][q]);
        }
        for (int p = 0; p < 4; ++p) {
            const int n = n0 + tr * 4 + p;
            if (n >= Nv) break;
            for (int q = 0; q < 4; ++q) {
                const float z = acc[p][q] + bc[q];
                if (z > vmax[q]) vmax[q] = z, jmax[q] = n;
                if (z < vmin[q]) vmin[q] = z, jmin[q] = n;
            }
        }
    }
    // combine the 16 row groups of each channel: largest (smallest) value, first row on ties
    __syncthreads();
    float *rv = &As[0][0];                     // [2][16][64] values
    int *ri = reinterpret_cast<int *>(&Ws[0][0]);  // [2][16][64] rows
    for (int q = 0; q < 4; ++q) {
        const int c = tc * 4 + q;
        rv[tr * PN_CB + c] = vmax[q], ri[tr * PN_CB + c] = jmax[q];
        rv[16 * PN_CB + tr * PN_CB + c] = vmin[q], ri[16 * PN_CB + tr * PN_CB + c] = jmin[q];
    }
    __syncthreads();
    if (t < PN_CB) {
        float bmax = rv[t], bmin = rv[16 * PN_CB + t];
        int imx = ri[t], imn = ri[16 * PN_CB + t];
        for (int g = 1; g < 16; ++g) {
            const float v1 = rv[g * PN_CB + t], v2 = rv[16 * PN_CB + g * PN_CB + t];
            const int i1 = ri[g * PN_CB + t], i2 = ri[16 * PN_CB + g * PN_CB + t];
            if (v1 > bmax || (v1 == bmax && i1 < imx)) bmax = v1, imx = i1;
            if (v2 < bmin || (v2 == bmin && i2 < imn)) bmin = v2, imn = i2;
        }
        const size_t o = (size_t)b * C + c0 + t;
        zmax[o] = bmax, imax[o] = imx, zmin[o] = bmin, imin[o] = imn;
    }
}

int launch_pn_pool_scan(const float *a, const int32_t *offs, const float *w, const float *bias, int B, int N, int K, int C, float *zmax,
                        int32_t *imax, float *zmin, int32_t *imin, hipStream_t st) {
    ProfScope ps(st, "pn_pool_scan_kernel B=%d N=%d K=%d C=%d", B, N, K, C);
    if (offs)
        hipLaunchKernelGGL(pn_pool_scan_kernel<true>, dim3(C / PN_CB, B), dim3(256), 0, st, a, offs, w, bias, N, K, C, zmax, imax, zmin, imin);
    else
        hipLaunchKernelGGL(pn_pool_scan_kernel<false>, dim3(C / PN_CB, B), dim3(256), 0, st, a, offs, w, bias, N, K, C, zmax, imax, zmin, imin);
    PNPP_CHECK_LAUNCH("pn_pool_scan");
    return PNPP_OK;
}

// ------------------------------------------------------------------------------------------------
// finalise: one wave per channel
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pn_pool_finalize_kernel(
    const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ gamma, const float *__restrict__ beta,
    const double *__restrict__ S, const double *__restrict__ Cc, const float *__restrict__ zmax, const int32_t *__restrict__ imax,
    const float *__restrict__ zmin, const int32_t *__restrict__ imin, int B, double M, int K, int C, int relu, int training, float eps,
    float momentum, float *rm, float *rv, long long *nbt, float *__restrict__ mean, float *__restrict__ istd_out,
    float *__restrict__ zsel, float *__restrict__ ypre, int32_t *__restrict__ route, float *__restrict__ out) {
    const int lane = threadIdx.x % 64, c = blockIdx.x * 4 + threadIdx.x / 64;
    if (training && nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
    if (c >= C) return;
    const float *wc = w + (size_t)c * K;
    double mu, var;
    if (training) {
        double ws = 0.0, q = 0.0;
        for (int i = lane; i < K; i += 64) {
            ws += (double)wc[i] * S[i];
            double ti = 0.0;
            for (int j = 0; j < K; ++j) ti += Cc[(size_t)i * K + j] * (double)wc[j];
            q += (double)wc[i] * ti;
        }
        ws = wave_sum(ws);
        q = wave_sum(q);
        mu = ws / M + (double)bias[c];
        var = q / M > 0.0 ? q / M : 0.0;
    } else {
        mu = rm[c];
        var = rv[c];
    }
    const float muf = (float)mu;
    const float istd = (float)(1.0 / sqrt(var + (double)eps));
    const float ac = gamma[c] * istd, bt = beta[c];
    for (int b = lane; b < B; b += 64) {
        const size_t o = (size_t)b * C + c;
        const bool up = ac >= 0.f;
        const float zs = up ? zmax[o] : zmin[o];
        const float y = (zs - muf) * ac + bt;
        zsel[o] = zs;
        ypre[o] = y;
        route[o] = up ? imax[o] : imin[o];
        out[o] = relu ? fmaxf(y, 0.f) : y;
    }
    if (lane == 0) {
        mean[c] = muf;
        istd_out[c] = istd;
        if (training) {
            rm[c] = (float)((1.0 - momentum) * (double)rm[c] + momentum * mu);
            rv[c] = (float)((1.0 - momentum) * (double)rv[c] + momentum * var * M / (M - 1.0));
        }
    }
}

int launch_pn_pool_finalize(const float *w, const float *bias, const float *gamma, const float *beta, const double *S, const double *Cc,
                            const float *zmax, const int32_t *imax, const float *zmin, const int32_t *imin, int B, long long M, int K, int C,
                            int relu, int training, float eps, float momentum, float *rm, float *rv, long long *nbt, float *mean,
                            float *istd, float *zsel, float *ypre, int32_t *route, float *out, hipStream_t st) {
    ProfScope ps(st, "pn_pool_finalize_kernel B=%d C=%d", B, C);
    hipLaunchKernelGGL(pn_pool_finalize_kernel, dim3(cdiv(C, 4)), dim3(256), 0, st, w, bias, gamma, beta, S, Cc, zmax, imax, zmin, imin,
                       B, (double)M, K, C, relu, training, eps, momentum, rm, rv, nbt, mean, istd, zsel, ypre, route, out);
    PNPP_CHECK_LAUNCH("pn_pool_finalize");
    return PNPP_OK;
}

// ------------------------------------------------------------------------------------------------
// backward, per channel (one wave each)
// ------------------------------------------------------------------------------------------------
template <bool RAGGED>
__global__ void __launch_bounds__(256) pn_pool_bwd_channels_kernel(
    const float *__restrict__ a, const int32_t *__restrict__ offs, double M, const float *__restrict__ w, const float *__restrict__ gamma, const float *__restrict__ dout,
    const float *__restrict__ mean, const float *__restrict__ istd, const float *__restrict__ zsel, const float *__restrict__ ypre,
    const int32_t *__restrict__ route, const double *__restrict__ S, const double *__restrict__ Cc, int B, int N, int K, int C, int relu,
    int training, float *__restrict__ dw, float *__restrict__ db, float *__restrict__ dgamma, float *__restrict__ dbeta,
    float *__restrict__ coef, float *__restrict__ u, float *__restrict__ v) {
    const int lane = threadIdx.x % 64, c = blockIdx.x * 4 + threadIdx.x / 64;
    if (c >= C) return;
    const float is = istd[c], mu = mean[c], ac = gamma[c] * is;
    double sh = 0.0, shx = 0.0;
    for (int b = lane; b < B; b += 64) {
        const size_t o = (size_t)b * C + c;
        const float h = (relu && !(ypre[o] > 0.f)) ? 0.f : dout[o];
        const float xh = (zsel[o] - mu) * is;
        sh += h;
        shx += (double)h * xh;
        coef[o] = ac * h;
    }
    sh = wave_sum(sh);
    shx = wave_sum(shx);
    const double gbar = sh / M, m = shx / M;
    if (lane == 0) {
        dgamma[c] = (float)shx;
        dbeta[c] = (float)sh;
        db[c] = training ? 0.f : (float)(ac * sh);
        u[c] = training ? (float)(ac * gbar) : 0.f;
        v[c] = training ? (float)(ac * m * is) : 0.f;
    }
    const float *wc = w + (size_t)c * K;
    for (int k = lane; k < K; k += 64) {
        double acc = 0.0;
        for (int b = 0; b < B; ++b) {
            const size_t o = (size_t)b * C + c;
            const float h = (relu && !(ypre[o] > 0.f)) ? 0.f : dout[o];
            const size_t row0 = RAGGED ? (size_t)offs[b] : (size_t)b * N;
            acc += (double)h * a[(row0 + route[o]) * K + k];
        }
        if (training) {
            double cw = 0.0;
            for (int j = 0; j < K; ++j) cw += Cc[(size_t)k * K + j] * (double)wc[j];
            acc = acc - gbar * S[k] - m * (double)is * cw;
        }
        dw[(size_t)c * K + k] = (float)(ac * acc);
    }
}

int launch_pn_pool_bwd_channels(const float *a, const int32_t *offs, long long M, const float *w, const float *gamma, const float *dout, const float *mean,
                                const float *istd, const float *zsel, const float *ypre, const int32_t *route, const double *S,
                                const double *Cc, int B, int N, int K, int C, int relu, int training, float *dw, float *db,
                                float *dgamma, float *dbeta, float *coef, float *u, float *v, hipStream_t st) {
    ProfScope ps(st, "pn_pool_bwd_channels_kernel B=%d K=%d C=%d", B, K, C);
    if (offs)
        hipLaunchKernelGGL(pn_pool_bwd_channels_kernel<true>, dim3(cdiv(C, 4)), dim3(256), 0, st, a, offs, (double)M, w, gamma, dout, mean,
                           istd, zsel, ypre, route, S, Cc, B, N, K, C, relu, training, dw, db, dgamma, dbeta, coef, u, v);
    else
        hipLaunchKernelGGL(pn_pool_bwd_channels_kernel<false>, dim3(cdiv(C, 4)), dim3(256), 0, st, a, offs, (double)M, w, gamma, dout, mean,
                           istd, zsel, ypre, route, S, Cc, B, N, K, C, relu, training, dw, db, dgamma, dbeta, coef, u, v);
    PNPP_CHECK_LAUNCH("pn_pool_bwd_channels");
    return PNPP_OK;
}

// Q = W^T diag(v) W (one row per workgroup) and cvec = -W^T u
__global__ void __launch_bounds__(PN_KMAX) pn_pool_bwd_q_kernel(const float *__restrict__ w, const float *__restrict__ u,
                                                                const float *__restrict__ v, int K, int C, float *__restrict__ Q,
                                                                float *__restrict__ cvec) {
    __shared__ double part[PN_KMAX];
    __shared__ float Wc[32][PN_KMAX];
    __shared__ float vc[32], uc[32];
    const int i = blockIdx.x, j = threadIdx.x;
    double q = 0.0, r = 0.0;
    for (int c0 = 0; c0 < C; c0 += 32) {   // 32 channels of W staged in LDS at a time (C is a multiple of 64)
        __syncthreads();
        for (int idx = j; idx < 32 * K; idx += PN_KMAX) Wc[idx / K][idx % K] = w[(size_t)(c0 + idx / K) * K + idx % K];
        if (j < 32) vc[j] = v[c0 + j], uc[j] = u[c0 + j];
        __syncthreads();
        if (j < K)
            for (int cc = 0; cc < 32; ++cc) q += (double)Wc[cc][i] * (double)vc[cc] * (double)Wc[cc][j];
        // W^T u split over the threads by channel, summed in a fixed order below
        if (j < 32) r += (double)Wc[j][i] * (double)uc[j];
    }
    part[j] = r;
    __syncthreads();
    if (j < K) Q[(size_t)i * K + j] = (float)q;
    if (j == 0) {
        double r0 = 0.0;
        for (int jj = 0; jj < PN_KMAX; ++jj) r0 += part[jj];
        cvec[i] = (float)(-r0);
    }
}

int launch_pn_pool_bwd_q(const float *w, const float *u, const float *v, int K, int C, float *Q, float *cvec, hipStream_t st) {
    ProfScope ps(st, "pn_pool_bwd_q_kernel K=%d C=%d", K, C);
    hipLaunchKernelGGL(pn_pool_bwd_q_kernel, dim3(K), dim3(PN_KMAX), 0, st, w, u, v, K, C, Q, cvec);
    PNPP_CHECK_LAUNCH("pn_pool_bwd_q");
    return PNPP_OK;
}

// dA for one (64-row tile, cloud): cvec - Q (A_n - S/M) (train; the tile is centred as it is loaded, so a column whose mean is large
// against its spread loses no digits), then the routed rows gathered in ascending channel order
template <bool RAGGED>
__global__ void __launch_bounds__(256) pn_pool_bwd_da_kernel(const float *__restrict__ a, const int32_t *__restrict__ offs,
                                                              const float *__restrict__ w,
                                                              const float *__restrict__ Q, const float *__restrict__ cvec,
                                                              const float *__restrict__ coef, const int32_t *__restrict__ route,
                                                              const double *__restrict__ S, double M, int N, int K, int C,
                                                              int training, float *__restrict__ da) {
    __shared__ __attribute__((aligned(16))) float Qs[PN_KMAX][PN_KMAX];
    __shared__ __attribute__((aligned(16))) float As[PN_KMAX * PN_RT];  // A tile [K][64] (k-major), then the output tile [64][K]
    __shared__ int ent_c[PN_CMAX];
    __shared__ short ent_r[PN_CMAX];
    __shared__ int cnt[257];
    __shared__ double mcol[PN_KMAX];
    const int n0 = blockIdx.x * PN_RT, b = blockIdx.y, t = threadIdx.x;
    size_t row0;
    int Nv;
    pn_cloud_rows<RAGGED>(offs, b, N, row0, Nv);
    if (RAGGED && n0 >= Nv) return;   // block-uniform, before the first barrier: no packed row belongs to this tile
    if (training && t < K) mcol[t] = S[t] / M;
    // 1. the (row, channel) pairs routed into this tile, in ascending channel order
    const int cpt = (C + 255) / 256;
    int mine = 0;
    for (int c = t * cpt; c < (t + 1) * cpt && c < C; ++c) {
        const int r = route[(size_t)b * C + c] - n0;
        mine += (r >= 0 && r < PN_RT);
    }
    cnt[t] = mine;
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int i = 0; i < 256; ++i) {
            const int x = cnt[i];
            cnt[i] = s;
            s += x;
        }
        cnt[256] = s;
    }
    __syncthreads();
    {
        int pos = cnt[t];
        for (int c = t * cpt; c < (t + 1) * cpt && c < C; ++c) {
            const int r = route[(size_t)b * C + c] - n0;
            if (r >= 0 && r < PN_RT) ent_c[pos] = c, ent_r[pos] = (short)r, ++pos;
        }
    }
    const int nent = cnt[256];
    const int tc = t % 16, tr = t / 16;
    float acc[4][8] = {};
    if (training) {
        for (int idx = t; idx < K * K; idx += 256) Qs[idx / K][idx % K] = Q[idx];
        for (int idx = t; idx < PN_RT * K; idx += 256) {
            const int r = idx / K, k = idx % K, n = n0 + r;
            As[k * PN_RT + r] = n < Nv ? (float)((double)a[(row0 + n) * K + k] - mcol[k]) : 0.f;
        }
        __syncthreads();
        if (tc * 8 < K)
            for (int j = 0; j < K; ++j) {
                const float4 av = *reinterpret_cast<const float4 *>(&As[j * PN_RT + tr * 4]);
                const float4 q0 = *reinterpret_cast<const float4 *>(&Qs[j][tc * 8]);
                const float4 q1 = *reinterpret_cast<const float4 *>(&Qs[j][tc * 8 + 4]);
                const float ar[4] = {av.x, av.y, av.z, av.w};
                const float qr[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                for (int p = 0; p < 4; ++p)
                    for (int q = 0; q < 8; ++q) acc[p][q] = fmaf(ar[p], qr[q], acc[p][q]);
            }
    }
    __syncthreads();
    float *Os = As;  // [64][K]
    for (int p = 0; p < 4; ++p)
        for (int q = 0; q < 8; ++q) {
            const int r = tr * 4 + p, k = tc * 8 + q;
            if (k < K) Os[r * K + k] = training ? cvec[k] - acc[p][q] : 0.f;
        }
    __syncthreads();
    // 2. R: each thread owns one column; entries in ascending channel order (deterministic, no atomics)
    if (t < K)
        for (int e = 0; e < nent; ++e) {
            const int c = ent_c[e], r = ent_r[e];
            Os[r * K + t] = fmaf(coef[(size_t)b * C + c], w[(size_t)c * K + t], Os[r * K + t]);
        }
    __syncthreads();
    for (int idx = t; idx < PN_RT * K; idx += 256) {
        const int r = idx / K, k = idx % K, n = n0 + r;
        if (n < Nv) da[(row0 + n) * K + k] = Os[idx];
    }
}

int launch_pn_pool_bwd_da(const float *a, const int32_t *offs, long long M, const float *w, const float *Q, const float *cvec, const float *coef, const int32_t *route,
                          const double *S, int B, int N, int K, int C, int training, float *da, hipStream_t st) {
    ProfScope ps(st, "pn_pool_bwd_da_kernel B=%d N=%d K=%d C=%d", B, N, K, C);
    if (offs)
        hipLaunchKernelGGL(pn_pool_bwd_da_kernel<true>, dim3(cdiv(N, PN_RT), B), dim3(256), 0, st, a, offs, w, Q, cvec, coef, route, S,
                           (double)M, N, K, C, training, da);
    else
        hipLaunchKernelGGL(pn_pool_bwd_da_kernel<false>, dim3(cdiv(N, PN_RT), B), dim3(256), 0, st, a, offs, w, Q, cvec, coef, route, S,
                           (double)M, N, K, C, training, da);
    PNPP_CHECK_LAUNCH("pn_pool_bwd_da");
    return PNPP_OK;
}

// ------------------------------------------------------------------------------------------------
// per-cloud transform
// ------------------------------------------------------------------------------------------------
// RAGGED: y holds packed rows; x is the padded input (row n of cloud b at b * sb + n * sn, rows n >= Nv never read) or, with xpacked,
// packed rows itself (row offs[b] + n at pitch sn: the feature transform of an already packed layer)
template <bool RAGGED>
__global__ void __launch_bounds__(256) pn_transform_kernel(const float *__restrict__ x, const int32_t *__restrict__ offs, int xpacked,
                                                            long long sb, long long sn, long long sd, const float *__restrict__ tm, int N,
                                                            int D, int k, int ldy, float *__restrict__ y) {
    __shared__ float Ts[PN_TMAX * PN_TMAX];
    __shared__ float Xs[PN_RT][PN_TMAX + 1];
    const int n0 = blockIdx.x * PN_RT, b = blockIdx.y, t = threadIdx.x;
    size_t row0;
    int Nv;
    pn_cloud_rows<RAGGED>(offs, b, N, row0, Nv);
    if (RAGGED && n0 >= Nv) return;   // block-uniform, before the first barrier
    const long long xb = (RAGGED && xpacked) ? (long long)row0 * sn : b * sb;
    if (tm)
        for (int idx = t; idx < k * k; idx += 256) Ts[idx] = tm[(size_t)b * k * k + idx];
    for (int idx = t; idx < PN_RT * D; idx += 256) {
        int r, d;
        if (sd == 1) r = idx / D, d = idx % D;
        else d = idx / PN_RT, r = idx % PN_RT;
        const int n = n0 + r;
        Xs[r][d] = n < Nv ? x[xb + n * sn + d * sd] : 0.f;
    }
    __syncthreads();
    for (int idx = t; idx < PN_RT * ldy; idx += 256) {
        const int r = idx / ldy, j = idx % ldy, n = n0 + r;
        if (n >= Nv) break;
        float val = 0.f;
        if (tm && j < k) {
            for (int i = 0; i < k; ++i) val = fmaf(Xs[r][i], Ts[i * k + j], val);
        } else if (j < D) {
            val = Xs[r][j];
        }
        y[(row0 + n) * ldy + j] = val;
    }
}

int launch_pn_transform(const float *x, const int32_t *offs, int xpacked, long long sb, long long sn, long long sd, const float *t, int B,
                        int N, int D, int k, int ldy, float *y, hipStream_t st) {
    ProfScope ps(st, "pn_transform_kernel N=%d D=%d k=%d", N, D, t ? k : 0);
    if (offs)
        hipLaunchKernelGGL(pn_transform_kernel<true>, dim3(cdiv(N, PN_RT), B), dim3(256), 0, st, x, offs, xpacked, sb, sn, sd, t, N, D, k, ldy,
                           y);
    else
        hipLaunchKernelGGL(pn_transform_kernel<false>, dim3(cdiv(N, PN_RT), B), dim3(256), 0, st, x, offs, 0, sb, sn, sd, t, N, D, k, ldy, y);
    PNPP_CHECK_LAUNCH("pn_transform");
    return PNPP_OK;
}

// dX_b = dY_b T_b^T on the transformed columns, the passed-through columns copied; written with X's strides
// RAGGED: dy holds packed rows; dx has the padded layout with exact zeros at rows n >= Nv, or (xpacked) the packed one
template <bool RAGGED>
__global__ void __launch_bounds__(256) pn_transform_dx_kernel(const float *__restrict__ tm, const float *__restrict__ dy,
                                                               const int32_t *__restrict__ offs, int xpacked, long long sb, long long sn,
                                                               long long sd, int N, int D, int k, int ldy, float *__restrict__ dx) {
    __shared__ float Ts[PN_TMAX * PN_TMAX];
    __shared__ float Ys[PN_RT][PN_TMAX + 1];
    const int n0 = blockIdx.x * PN_RT, b = blockIdx.y, t = threadIdx.x;
    size_t row0;
    int Nv;
    pn_cloud_rows<RAGGED>(offs, b, N, row0, Nv);
    const long long xb = (RAGGED && xpacked) ? (long long)row0 * sn : b * sb;
    if (RAGGED && n0 >= Nv) {   // block-uniform, before the first barrier: a tile of padding rows alone
        if (!xpacked)
            for (int idx = t; idx < PN_RT * D; idx += 256) {
                int r, i;
                if (sd == 1) r = idx / D, i = idx % D;
                else i = idx / PN_RT, r = idx % PN_RT;
                if (n0 + r < N) dx[xb + (n0 + r) * sn + i * sd] = 0.f;
            }
        return;
    }
    if (tm)
        for (int idx = t; idx < k * k; idx += 256) Ts[idx] = tm[(size_t)b * k * k + idx];
    for (int idx = t; idx < PN_RT * D; idx += 256) {
        const int r = idx / D, j = idx % D, n = n0 + r;
        Ys[r][j] = n < Nv ? dy[(row0 + n) * ldy + j] : 0.f;
    }
    __syncthreads();
    for (int idx = t; idx < PN_RT * D; idx += 256) {
        int r, i;
        if (sd == 1) r = idx / D, i = idx % D;
        else i = idx / PN_RT, r = idx % PN_RT;
        const int n = n0 + r;
        if (n >= ((RAGGED && !xpacked) ? N : Nv)) continue;
        float val;
        if (RAGGED && n >= Nv) {
            val = 0.f;
        } else if (tm && i < k) {
            val = 0.f;
            for (int j = 0; j < k; ++j) val = fmaf(Ys[r][j], Ts[i * k + j], val);
        } else {
            val = Ys[r][i];
        }
        dx[xb + n * sn + i * sd] = val;
    }
}

// dT_b = X_b^T dY_b over the cloud's rows, float64, slices of rows summed in a fixed order
template <bool RAGGED>
__global__ void __launch_bounds__(256) pn_transform_dt_kernel(const float *__restrict__ x, const int32_t *__restrict__ offs, int xpacked,
                                                               long long sb, long long sn, long long sd, const float *__restrict__ dy, int N,
                                                               int k, int ldy, int epw, float *__restrict__ dt) {
    __shared__ double red[256];
    const int b = blockIdx.y, t = threadIdx.x;
    size_t row0;
    int Nv;
    pn_cloud_rows<RAGGED>(offs, b, N, row0, Nv);
    const long long xb = (RAGGED && xpacked) ? (long long)row0 * sn : b * sb;
    const int e = blockIdx.x * epw + t % epw, s = t / epw, nslice = 256 / epw;
    double acc = 0.0;
    if (e < k * k) {
        const int i = e / k, j = e % k;
        for (int n = s; n < Nv; n += nslice)
            acc += (double)x[xb + n * sn + i * sd] * (double)dy[(row0 + n) * ldy + j];
    }
    red[t] = acc;
    __syncthreads();
    if (s == 0 && e < k * k) {
        double tot = 0.0;
        for (int q = 0; q < nslice; ++q) tot += red[q * epw + t];
        dt[(size_t)b * k * k + e] = (float)tot;
    }
}

int launch_pn_transform_bwd(const float *x, const int32_t *offs, int xpacked, long long sb, long long sn, long long sd, const float *t,
                            const float *dy, int B, int N, int D, int k, int ldy, float *dx, float *dt, hipStream_t st) {
    if (dx) {
        ProfScope ps(st, "pn_transform_dx_kernel N=%d D=%d k=%d", N, D, t ? k : 0);
        if (offs)
            hipLaunchKernelGGL(pn_transform_dx_kernel<true>, dim3(cdiv(N, PN_RT), B), dim3(256), 0, st, t, dy, offs, xpacked, sb, sn, sd, N, D, k,
                               ldy, dx);
        else
            hipLaunchKernelGGL(pn_transform_dx_kernel<false>, dim3(cdiv(N, PN_RT), B), dim3(256), 0, st, t, dy, offs, 0, sb, sn, sd, N, D, k, ldy,
                               dx);
        PNPP_CHECK_LAUNCH("pn_transform_dx");
    }
    if (dt) {
        int epw = 1;
        while (epw < k * k && epw < 256) epw *= 2;
        ProfScope ps(st, "pn_transform_dt_kernel N=%d k=%d", N, k);
        if (offs)
            hipLaunchKernelGGL(pn_transform_dt_kernel<true>, dim3(cdiv(k * k, epw), B), dim3(256), 0, st, x, offs, xpacked, sb, sn, sd, dy, N, k,
                               ldy, epw, dt);
        else
            hipLaunchKernelGGL(pn_transform_dt_kernel<false>, dim3(cdiv(k * k, epw), B), dim3(256), 0, st, x, offs, 0, sb, sn, sd, dy, N, k, ldy,
                               epw, dt);
        PNPP_CHECK_LAUNCH("pn_transform_dt");
    }
    return PNPP_OK;
}

// ------------------------------------------------------------------------------------------------
// regulariser
// ------------------------------------------------------------------------------------------------
__device__ inline double block_sum256(double v, double *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(256) pn_reg_norm_kernel(const float *__restrict__ tm, int k, double *__restrict__ norms) {
    __shared__ float Ts[PN_TMAX * PN_TMAX];
    __shared__ double red[256];
    const int b = blockIdx.x, t = threadIdx.x;
    for (int idx = t; idx < k * k; idx += 256) Ts[idx] = tm[(size_t)b * k * k + idx];
    __syncthreads();
    double acc = 0.0;
    for (int e = t; e < k * k; e += 256) {
        const int i = e / k, j = e % k;
        double v = (i == j) ? -1.0 : 0.0;
        for (int l = 0; l < k; ++l) v += (double)Ts[i * k + l] * (double)Ts[j * k + l];
        acc += v * v;
    }
    const double s = block_sum256(acc, red);
    if (t == 0) norms[b] = sqrt(s);
}

__global__ void pn_reg_mean_kernel(const double *__restrict__ norms, int B, float *__restrict__ out) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += norms[b];
    out[0] = (float)(s / B);
}

int launch_pn_regularizer(const float *t, int B, int k, double *norms, float *out, hipStream_t st) {
    {
        ProfScope ps(st, "pn_reg_norm_kernel B=%d k=%d", B, k);
        hipLaunchKernelGGL(pn_reg_norm_kernel, dim3(B), dim3(256), 0, st, t, k, norms);
        PNPP_CHECK_LAUNCH("pn_reg_norm");
    }
    ProfScope ps(st, "pn_reg_mean_kernel B=%d", B);
    hipLaunchKernelGGL(pn_reg_mean_kernel, dim3(1), dim3(64), 0, st, norms, B, out);
    PNPP_CHECK_LAUNCH("pn_reg_mean");
    return PNPP_OK;
}

// dT_b = dout * 2 (T_b T_b^T - I) T_b / (B ||.||_F)
__global__ void __launch_bounds__(256) pn_reg_bwd_kernel(const float *__restrict__ tm, const double *__restrict__ norms,
                                                          const float *__restrict__ dout, int B, int k, float *__restrict__ dt) {
    __shared__ float Ts[PN_TMAX * PN_TMAX];
    __shared__ double Es[PN_TMAX * PN_TMAX];
    const int b = blockIdx.x, t = threadIdx.x;
    for (int idx = t; idx < k * k; idx += 256) Ts[idx] = tm[(size_t)b * k * k + idx];
    __syncthreads();
    for (int e = t; e < k * k; e += 256) {
        const int i = e / k, j = e % k;
        double v = (i == j) ? -1.0 : 0.0;
        for (int l = 0; l < k; ++l) v += (double)Ts[i * k + l] * (double)Ts[j * k + l];
        Es[e] = v;
    }
    __syncthreads();
    const double nb = norms[b];
    const double sc = nb > 0.0 ? 2.0 * (double)dout[0] / ((double)B * nb) : 0.0;
    for (int e = t; e < k * k; e += 256) {
        const int i = e / k, j = e % k;
        double v = 0.0;
        for (int l = 0; l < k; ++l) v += Es[i * k + l] * (double)Ts[l * k + j];
        dt[(size_t)b * k * k + e] = (float)(sc * v);
    }
}

int launch_pn_regularizer_bwd(const float *t, const double *norms, const float *dout, int B, int k, float *dt, hipStream_t st) {
    ProfScope ps(st, "pn_reg_bwd_kernel B=%d k=%d", B, k);
    hipLaunchKernelGGL(pn_reg_bwd_kernel, dim3(B), dim3(256), 0, st, t, norms, dout, B, k, dt);
    PNPP_CHECK_LAUNCH("pn_reg_bwd");
    return PNPP_OK;
}

// ------------------------------------------------------------------------------------------------
// heads and encoder output
// ------------------------------------------------------------------------------------------------
__global__ void pn_add_identity_kernel(const float *__restrict__ x, int B, int k, float *__restrict__ y) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * k * k) return;
    const int e = (int)(idx % (k * k));
    y[idx] = x[idx] + ((e / k == e % k) ? 1.f : 0.f);
}

int launch_pn_add_identity(const float *x, int B, int k, float *y, hipStream_t st) {
    ProfScope ps(st, "pn_add_identity_kernel B=%d k=%d", B, k);
    hipLaunchKernelGGL(pn_add_identity_kernel, dim3(cdiv(B * k * k, 256)), dim3(256), 0, st, x, B, k, y);
    PNPP_CHECK_LAUNCH("pn_add_identity");
    return PNPP_OK;
}

// out (B, C1 + C2, N): rows 0..C1-1 the global feature repeated over the points, then the per-point features (rows of pf)
// RAGGED: pf holds packed rows (or, pf_padded, padded ones: the Predictor's tapped features); columns n >= Nv of out are exact zeros
template <bool RAGGED>
__global__ void pn_concat_kernel(const float *__restrict__ g, const float *__restrict__ pf, const int32_t *__restrict__ offs, int pf_padded,
                                 int B, int N, int C1, int C2, float *__restrict__ out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Ct = C1 + C2;
    if (idx >= (long long)B * Ct * N) return;
    const int n = (int)(idx % N), c = (int)((idx / N) % Ct), b = (int)(idx / ((long long)N * Ct));
    size_t row0 = (size_t)b * N;
    if (RAGGED) {
        const int o0 = offs[b], Nv = min(max(offs[b + 1] - o0, 0), N);
        if (n >= Nv) {
            out[idx] = 0.f;
            return;
        }
        if (!pf_padded) row0 = (size_t)o0;
    }
    out[idx] = c < C1 ? g[(size_t)b * C1 + c] : pf[(row0 + n) * C2 + (c - C1)];
}

// RAGGED: dout at columns n >= Nv is not read
template <bool RAGGED>
__global__ void __launch_bounds__(256) pn_concat_dg_kernel(const float *__restrict__ dout, const int32_t *__restrict__ offs, int N, int C1,
                                                            int C2, float *__restrict__ dg) {
    const int lane = threadIdx.x % 64, c = blockIdx.x * 4 + threadIdx.x / 64, b = blockIdx.y;
    if (c >= C1) return;
    const float *row = dout + ((size_t)b * (C1 + C2) + c) * N;
    double s = 0.0;
    size_t row0;
    int Nv;
    pn_cloud_rows<RAGGED>(offs, b, N, row0, Nv);
    for (int n = lane; n < Nv; n += 64) s += row[n];
    s = wave_sum_to0(s);
    if (lane == 0) dg[(size_t)b * C1 + c] = (float)s;
}

template <bool RAGGED>
__global__ void pn_concat_dpf_kernel(const float *__restrict__ dout, const int32_t *__restrict__ offs, int B, int N, int C1, int C2,
                                     float *__restrict__ dpf) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * N * C2) return;
    const int j = (int)(idx % C2), n = (int)((idx / C2) % N), b = (int)(idx / ((long long)C2 * N));
    if (RAGGED) {   // the grid covers the padded rows; the valid ones go to their packed places
        const int o0 = offs[b], Nv = min(max(offs[b + 1] - o0, 0), N);
        if (n < Nv) dpf[((size_t)o0 + n) * C2 + j] = dout[((size_t)b * (C1 + C2) + C1 + j) * N + n];
        return;
    }
    dpf[idx] = dout[((size_t)b * (C1 + C2) + C1 + j) * N + n];
}

int launch_pn_concat(const float *g, const float *pf, const int32_t *offs, int pf_padded, int B, int N, int C1, int C2, float *out,
                     hipStream_t st) {
    const long long tot = (long long)B * (C1 + C2) * N;
    ProfScope ps(st, "pn_concat_kernel B=%d N=%d", B, N);
    if (offs)
        hipLaunchKernelGGL(pn_concat_kernel<true>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, g, pf, offs, pf_padded, B, N, C1, C2,
                           out);
    else
        hipLaunchKernelGGL(pn_concat_kernel<false>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, g, pf, offs, 0, B, N, C1, C2, out);
    PNPP_CHECK_LAUNCH("pn_concat");
    return PNPP_OK;
}

int launch_pn_concat_bwd(const float *dout, const int32_t *offs, int B, int N, int C1, int C2, float *dg, float *dpf, hipStream_t st) {
    if (dg) {
        ProfScope ps(st, "pn_concat_dg_kernel B=%d N=%d", B, N);
        if (offs)
            hipLaunchKernelGGL(pn_concat_dg_kernel<true>, dim3(cdiv(C1, 4), B), dim3(256), 0, st, dout, offs, N, C1, C2, dg);
        else
            hipLaunchKernelGGL(pn_concat_dg_kernel<false>, dim3(cdiv(C1, 4), B), dim3(256), 0, st, dout, offs, N, C1, C2, dg);
        PNPP_CHECK_LAUNCH("pn_concat_dg");
    }
    if (dpf) {
        const long long tot = (long long)B * N * C2;
        ProfScope ps(st, "pn_concat_dpf_kernel B=%d N=%d", B, N);
        if (offs)
            hipLaunchKernelGGL(pn_concat_dpf_kernel<true>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, dout, offs, B, N, C1, C2, dpf);
        else
            hipLaunchKernelGGL(pn_concat_dpf_kernel<false>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, dout, offs, B, N, C1, C2, dpf);
        PNPP_CHECK_LAUNCH("pn_concat_dpf");
    }
    return PNPP_OK;
}

// BatchNorm1d + ReLU over (M, C) rows on its own: the PointNet head's bn2 sits AFTER the dropout (relu(bn2(dropout(fc2(x)))))
__global__ void pn_bn_relu_kernel(const float *__restrict__ x, int M, int C, const float *__restrict__ gamma,
                                  const float *__restrict__ beta, float *rm, float *rv, long long *nbt, int training, float eps,
                                  float momentum, float *__restrict__ mean, float *__restrict__ istd_out, float *__restrict__ y) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (training && nbt && c == 0) *nbt += 1;
    if (c >= C) return;
    double mu, var;
    if (training) {
        double s = 0.0, s2 = 0.0;
        for (int m = 0; m < M; ++m) s += x[(size_t)m * C + c];
        mu = s / M;
        for (int m = 0; m < M; ++m) {
            const double d = x[(size_t)m * C + c] - mu;
            s2 += d * d;
        }
        var = s2 / M;
        rm[c] = (float)((1.0 - momentum) * (double)rm[c] + momentum * mu);
        rv[c] = (float)((1.0 - momentum) * (double)rv[c] + momentum * var * M / (M - 1.0));
    } else {
        mu = rm[c];
        var = rv[c];
    }
    const float muf = (float)mu, is = (float)(1.0 / sqrt(var + (double)eps)), ga = gamma[c], be = beta[c];
    mean[c] = muf;
    istd_out[c] = is;
    for (int m = 0; m < M; ++m) y[(size_t)m * C + c] = fmaxf((x[(size_t)m * C + c] - muf) * is * ga + be, 0.f);
}

__global__ void pn_bn_relu_bwd_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ dy, int M,
                                      int C, const float *__restrict__ gamma, const float *__restrict__ mean,
                                      const float *__restrict__ istd, int training, float *__restrict__ dx,
                                      float *__restrict__ dgamma, float *__restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float mu = mean[c], is = istd[c], ga = gamma[c];
    double sh = 0.0, shx = 0.0;
    for (int m = 0; m < M; ++m) {
        const size_t o = (size_t)m * C + c;
        const float h = y[o] > 0.f ? dy[o] : 0.f;
        sh += h;
        shx += (double)h * ((x[o] - mu) * is);
    }
    dgamma[c] = (float)shx;
    dbeta[c] = (float)sh;
    if (!dx) return;
    const double gbar = sh / M, mm = shx / M;
    for (int m = 0; m < M; ++m) {
        const size_t o = (size_t)m * C + c;
        const double h = y[o] > 0.f ? dy[o] : 0.f;
        const double xh = (double)((x[o] - mu) * is);
        dx[o] = training ? (float)((double)ga * is * (h - gbar - xh * mm)) : (float)((double)ga * is * h);
    }
}

int launch_pn_bn_relu(const float *x, int M, int C, const float *gamma, const float *beta, float *rm, float *rv, long long *nbt,
                      int training, float eps, float momentum, float *mean, float *istd, float *y, hipStream_t st) {
    ProfScope ps(st, "pn_bn_relu_kernel M=%d C=%d", M, C);
    hipLaunchKernelGGL(pn_bn_relu_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, x, M, C, gamma, beta, rm, rv, nbt, training, eps,
                       momentum, mean, istd, y);
    PNPP_CHECK_LAUNCH("pn_bn_relu");
    return PNPP_OK;
}

int launch_pn_bn_relu_bwd(const float *x, const float *y, const float *dy, int M, int C, const float *gamma, const float *mean,
                          const float *istd, int training, float *dx, float *dgamma, float *dbeta, hipStream_t st) {
    ProfScope ps(st, "pn_bn_relu_bwd_kernel M=%d C=%d", M, C);
    hipLaunchKernelGGL(pn_bn_relu_bwd_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, x, y, dy, M, C, gamma, mean, istd, training, dx,
                       dgamma, dbeta);
    PNPP_CHECK_LAUNCH("pn_bn_relu_bwd");
    return PNPP_OK;
}

}  // namespace pnpp
