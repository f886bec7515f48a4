// cls_loss_kernels.hip -- the classification head of PointNet++Demo.py: F.log_softmax(x, dim=1) (:234) and F.nll_loss(pred, target) (:244),
// forward and backward, and the forward-only tail  log_softmax(x W^T + b)  of the classifier's Predictor as one launch.
//
// One wave owns a row.  The row maximum and the sums are wave reductions (xor butterflies: every lane ends with the same value, the
// order of the additions is fixed by the lane count, so two runs agree bit for bit); sums accumulate in float64 like the other loss
// kernels (soft_ce_kernel, mse_rows_kernel) and are rounded once.  A row is read from global memory three times instead of being
// held in registers: any C is taken, and a row of a classifier (40 ... 1000 floats) stays in the L1 after the first pass.
#include "kernels.h"

namespace pnpp {
namespace {

constexpr int kRowsPerBlock = 4;   // waves per workgroup
constexpr int kLinLsMaxC = 1024;   // linear_log_softmax keeps C / 64 logits per lane in registers

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_f64(v, m);
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// y[m, c] = x[m, c] - (max_c x + log sum_c exp(x - max))
__global__ void __launch_bounds__(64 * kRowsPerBlock) log_softmax_kernel(const float *__restrict__ x, int M, int C, float *__restrict__ y) {
    const int m = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6), lane = lane_id();
    if (m >= M) return;   // wave-uniform
    const float *xr = x + (size_t)m * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, xr[c]);
    mx = wave_max_f32(mx);
    double se = 0.0;
    for (int c = lane; c < C; c += 64) se += exp((double)xr[c] - (double)mx);
    const double lse = (double)mx + log(wave_sum_f64(se));
    for (int c = lane; c < C; c += 64) y[(size_t)m * C + c] = (float)((double)xr[c] - lse);
}

// dx[m, c] = dy[m, c] - exp(y[m, c]) * sum_c dy[m, c]
__global__ void __launch_bounds__(64 * kRowsPerBlock) log_softmax_bwd_kernel(const float *__restrict__ y, const float *__restrict__ dy, int M,
                                                                             int C, float *__restrict__ dx) {
    const int m = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6), lane = lane_id();
    if (m >= M) return;
    const size_t r = (size_t)m * C;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)dy[r + c];
    s = wave_sum_f64(s);
    for (int c = lane; c < C; c += 64) dx[r + c] = (float)((double)dy[r + c] - exp((double)y[r + c]) * s);
}

// y[m, :] = log_softmax(x[m, :] W^T + b): lane l of the row's wave owns the logits c = l, l + 64, ...; float64 accumulation
template <int NC>
__global__ void __launch_bounds__(64 * kRowsPerBlock) linear_log_softmax_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                                const float *__restrict__ b, int M, int K, int C,
                                                                                float *__restrict__ y) {
    const int m = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6), lane = lane_id();
    if (m >= M) return;
    const float *xr = x + (size_t)m * K;
    double z[NC];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        z[i] = 0.0;
        if (c < C) {
            const float *wr = w + (size_t)c * K;
            double acc = (double)b[c];
            for (int k = 0; k < K; ++k) acc += (double)xr[k] * (double)wr[k];
            z[i] = (double)(float)acc;   // the logit as the float32 tensor the unfused path would hand to log_softmax
            mx = fmaxf(mx, (float)acc);
        }
    }
    mx = wave_max_f32(mx);
    double se = 0.0;
#pragma unroll
    for (int i = 0; i < NC; ++i)
        if (lane + 64 * i < C) se += exp(z[i] - (double)mx);
    const double lse = (double)mx + log(wave_sum_f64(se));
#pragma unroll
    for (int i = 0; i < NC; ++i)
        if (lane + 64 * i < C) y[(size_t)m * C + lane + 64 * i] = (float)(z[i] - lse);
}

// loss_mean[0] = -(1/M) sum_m logp[m, target[m]]; bad[0] = the number of targets outside [0, C) (their rows add nothing).
// One workgroup, fixed-order float64 sum (pnpp_mse's scheme).
__global__ void __launch_bounds__(256) nll_loss_kernel(const float *__restrict__ logp, const int32_t *__restrict__ target, int M, int C,
                                                       float *__restrict__ loss_mean, int32_t *__restrict__ bad) {
    __shared__ double red[256];
    __shared__ int nbad[256];
    double acc = 0.0;
    int nb = 0;
    for (int m = threadIdx.x; m < M; m += 256) {
        const int t = target[m];
        if (t >= 0 && t < C) acc -= (double)logp[(size_t)m * C + t];
        else ++nb;
    }
    red[threadIdx.x] = acc, nbad[threadIdx.x] = nb;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s], nbad[threadIdx.x] += nbad[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss_mean[0] = (float)(red[0] / (double)M);
        bad[0] = nbad[0];
    }
}

// dlogp[m, c] = -g / M at c == target[m], else 0 (g: the upstream gradient of the mean, a device scalar)
__global__ void __launch_bounds__(256) nll_loss_bwd_kernel(const int32_t *__restrict__ target, const float *__restrict__ g, int M, int C,
                                                           float *__restrict__ dlogp) {
    const float v = -g[0] / (float)M;
    const size_t n = (size_t)M * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int m = (int)(i / C), c = (int)(i - (size_t)m * C);
        dlogp[i] = c == target[m] ? v : 0.f;
    }
}

}  // namespace
}  // namespace pnpp

using namespace pnpp;

extern "C" int pnpp_log_softmax(const float *x, int M, int C, float *y, void *stream) {
    PNPP_REQUIRE(x && y, PNPP_ERR_ARG, "log_softmax: null pointer");
    PNPP_REQUIRE(M > 0 && C > 0, PNPP_ERR_ARG, "log_softmax: non-positive size M=%d C=%d", M, C);
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, "log_softmax_kernel M=%d C=%d", M, C);
    hipLaunchKernelGGL(log_softmax_kernel, dim3(cdiv(M, kRowsPerBlock)), dim3(64 * kRowsPerBlock), 0, st, x, M, C, y);
    PNPP_CHECK_LAUNCH("log_softmax");
    return PNPP_OK;
}

extern "C" int pnpp_log_softmax_bwd(const float *y, const float *dy, int M, int C, float *dx, void *stream) {
    PNPP_REQUIRE(y && dy && dx, PNPP_ERR_ARG, "log_softmax_bwd: null pointer");
    PNPP_REQUIRE(M > 0 && C > 0, PNPP_ERR_ARG, "log_softmax_bwd: non-positive size M=%d C=%d", M, C);
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, "log_softmax_bwd_kernel M=%d C=%d", M, C);
    hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3(cdiv(M, kRowsPerBlock)), dim3(64 * kRowsPerBlock), 0, st, y, dy, M, C, dx);
    PNPP_CHECK_LAUNCH("log_softmax_bwd");
    return PNPP_OK;
}

extern "C" int pnpp_linear_log_softmax(const float *x, const float *w, const float *b, int M, int K, int C, float *y, void *stream) {
    PNPP_REQUIRE(x && w && b && y, PNPP_ERR_ARG, "linear_log_softmax: null pointer");
    PNPP_REQUIRE(M > 0 && K > 0 && C > 0, PNPP_ERR_ARG, "linear_log_softmax: non-positive size M=%d K=%d C=%d", M, K, C);
    PNPP_REQUIRE(C <= kLinLsMaxC, PNPP_ERR_ARG, "linear_log_softmax: C=%d classes exceed %d", C, kLinLsMaxC);
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, "linear_log_softmax_kernel M=%d K=%d C=%d", M, K, C);
    const dim3 grid(cdiv(M, kRowsPerBlock)), block(64 * kRowsPerBlock);
    if (C <= 64) hipLaunchKernelGGL(linear_log_softmax_kernel<1>, grid, block, 0, st, x, w, b, M, K, C, y);
    else if (C <= 256) hipLaunchKernelGGL(linear_log_softmax_kernel<4>, grid, block, 0, st, x, w, b, M, K, C, y);
    else hipLaunchKernelGGL(linear_log_softmax_kernel<16>, grid, block, 0, st, x, w, b, M, K, C, y);
    PNPP_CHECK_LAUNCH("linear_log_softmax");
    return PNPP_OK;
}

extern "C" int pnpp_nll_loss(const float *logp, const int32_t *target, int M, int C, float *loss_mean, int32_t *bad_targets, int check,
                             void *stream) {
    PNPP_REQUIRE(logp && target && loss_mean && bad_targets, PNPP_ERR_ARG, "nll_loss: null pointer");
    PNPP_REQUIRE(M > 0 && C > 0, PNPP_ERR_ARG, "nll_loss: non-positive size M=%d C=%d", M, C);
    hipStream_t st = as_stream(stream);
    {
        ProfScope ps(st, "nll_loss_kernel M=%d C=%d", M, C);
        hipLaunchKernelGGL(nll_loss_kernel, dim3(1), dim3(256), 0, st, logp, target, M, C, loss_mean, bad_targets);
        PNPP_CHECK_LAUNCH("nll_loss");
    }
    if (check) {   // the targets live on the device: their range is known only after the kernel has looked at them
        int32_t nbad = 0;
        hipError_t e = hipMemcpyAsync(&nbad, bad_targets, sizeof(nbad), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        PNPP_REQUIRE(e == hipSuccess, PNPP_ERR_LAUNCH, "nll_loss: reading the target check failed: %s", hipGetErrorString(e));
        PNPP_REQUIRE(nbad == 0, PNPP_ERR_RANGE, "nll_loss: %d of %d targets lie outside [0, %d)", (int)nbad, M, C);
    }
    return PNPP_OK;
}

extern "C" int pnpp_nll_loss_bwd(const int32_t *target, const float *grad_loss, int M, int C, float *dlogp, void *stream) {
    PNPP_REQUIRE(target && grad_loss && dlogp, PNPP_ERR_ARG, "nll_loss_bwd: null pointer");
    PNPP_REQUIRE(M > 0 && C > 0, PNPP_ERR_ARG, "nll_loss_bwd: non-positive size M=%d C=%d", M, C);
    hipStream_t st = as_stream(stream);
    const size_t n = (size_t)M * C;
    const int grid = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    ProfScope ps(st, "nll_loss_bwd_kernel M=%d C=%d", M, C);
    hipLaunchKernelGGL(nll_loss_bwd_kernel, dim3(grid), dim3(256), 0, st, target, grad_loss, M, C, dlogp);
    PNPP_CHECK_LAUNCH("nll_loss_bwd");
    return PNPP_OK;
}
