// optim_kernels.hip -- the flat-buffer optimiser: Adam with the step count on the host or in device memory, gradient clipping by the
// buffer's sum of squares (reduced on the device, read by the update: no host round trip).
#include "kernels.h"

namespace pnpp {

// ---- flat-buffer Adam (torch.optim.Adam defaults: no amsgrad, no weight decay) ---------------------
// torch.nn.utils.clip_grad_norm_(params, max_norm) (train_multi_peaks_vonMises_KL.py:235) folded into the update: sumsq[0]
// is the sum of squares of the flat gradient buffer as it stands (pnpp_sumsq), gscale the factor that turns the buffer into
// the gradient (1/world under data parallelism), so the gradient's norm is sqrt(sumsq) * gscale and the coefficient is
// min(1, max_norm / (norm + 1e-6)), torch's formula.  A null sumsq means no clipping.  No host round trip.
__device__ __forceinline__ float clip_coef(const double *__restrict__ sumsq, float gscale, float max_norm) {
    if (!sumsq) return 1.f;
    const float norm = (float)(sqrt(sumsq[0]) * (double)gscale);
    return fminf(1.f, max_norm / (norm + 1e-6f));
}
template <bool ZERO>
__global__ void __launch_bounds__(256) adam_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m,
                                                   float *__restrict__ v, size_t n, float lr_over_bc1, float inv_sqrt_bc2,
                                                   float b1, float b2, float eps, float gscale,
                                                   const double *__restrict__ sumsq, float max_norm) {
    gscale *= clip_coef(sumsq, gscale, max_norm);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float gi = g[i] * gscale;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= lr_over_bc1 * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
        if (ZERO) g[i] = 0.f;  // the next iteration's opt.zero_grad(), folded in
    }
}

// The same update with the step count in device memory, for launches that are captured in a hipGraph: state[0] = steps
// taken so far, state[1] = ticket.  Every workgroup reads state[0] before it takes its ticket and the last one
// advances the count, so each replay applies its own bias correction.  zero_grad != 0 clears every gradient once it has
// been consumed (the next step's zero_grad() memset, folded in).
__global__ void __launch_bounds__(256) adam_dev_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m,
                                                       float *__restrict__ v, size_t n, float lr, float b1, float b2, float eps,
                                                       float gscale, unsigned long long *__restrict__ state, int zero_grad,
                                                       const double *__restrict__ sumsq, float max_norm) {
    gscale *= clip_coef(sumsq, gscale, max_norm);
    __shared__ float bc[2];
    __shared__ unsigned long long step_s;
    if (threadIdx.x == 0) {
        const unsigned long long step = state[0] + 1ull;
        step_s = step;
        const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
        bc[0] = (float)((double)lr / bc1);
        bc[1] = (float)(1.0 / sqrt(bc2));
    }
    __syncthreads();
    const float lr_over_bc1 = bc[0], inv_sqrt_bc2 = bc[1];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float gi = g[i] * gscale;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= lr_over_bc1 * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
        if (zero_grad) g[i] = 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = atomicAdd(&state[1], 1ull);
        if (t == (unsigned long long)gridDim.x - 1ull) {
            state[1] = 0ull;
            state[0] = step_s;
        }
    }
}

__global__ void __launch_bounds__(256) sumsq_partial_kernel(const float *__restrict__ x, size_t n, double *__restrict__ part) {
    __shared__ double red[4];
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) acc += (double)x[i] * (double)x[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += shfl_xor_f64(acc, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void __launch_bounds__(64) sumsq_final_kernel(const double *__restrict__ part, int nb, double *__restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 64) acc += part[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += shfl_xor_f64(acc, m);
    if (threadIdx.x == 0) out[0] = acc;
}

}  // namespace pnpp

using namespace pnpp;

// One update of the flat buffers.  The step count is the host's (step > 0, state null: the bias correction is computed here) or lives
// in device memory (state).  sumsq null: no clipping.
struct AdamLaunch {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    size_t n;
    float lr, beta1, beta2, eps, grad_scale;
    int step;
    uint64_t *state;
    const double *sumsq;
    float max_norm;
    int zero_grad;
};

static void launch_adam(const AdamLaunch &a, void *stream) {
    const int grid = (int)((a.n + 255) / 256 < 2048 ? (a.n + 255) / 256 : 2048);
    if (a.state) {
        hipLaunchKernelGGL(adam_dev_kernel, dim3(grid), dim3(256), 0, as_stream(stream), a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n, a.lr,
                           a.beta1, a.beta2, a.eps, a.grad_scale, reinterpret_cast<unsigned long long *>(a.state), a.zero_grad, a.sumsq,
                           a.max_norm);
        return;
    }
    const double bc1 = 1.0 - pow((double)a.beta1, a.step), bc2 = 1.0 - pow((double)a.beta2, a.step);
    const auto kernel = a.zero_grad ? adam_kernel<true> : adam_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, as_stream(stream), a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n,
                       (float)((double)a.lr / bc1), (float)(1.0 / sqrt(bc2)), a.beta1, a.beta2, a.eps, a.grad_scale, a.sumsq, a.max_norm);
}

extern "C" int pnpp_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, int step, float lr,
                              float beta1, float beta2, float eps, float grad_scale, void *stream) {
    PNPP_REQUIRE(param && grad && exp_avg && exp_avg_sq, PNPP_ERR_ARG, "adam_step: null pointer");
    PNPP_REQUIRE(n > 0 && step > 0, PNPP_ERR_ARG, "adam_step: n and step must be positive");
    launch_adam({param, const_cast<float *>(grad), exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, grad_scale, step, nullptr, nullptr, 0.f, 0},
                stream);
    PNPP_CHECK_LAUNCH("adam_step");
    return PNPP_OK;
}

extern "C" int pnpp_adam_step_zero(float *param, float *grad, float *exp_avg, float *exp_avg_sq, size_t n, int step, float lr,
                                   float beta1, float beta2, float eps, float grad_scale, void *stream) {
    PNPP_REQUIRE(param && grad && exp_avg && exp_avg_sq, PNPP_ERR_ARG, "adam_step_zero: null pointer");
    PNPP_REQUIRE(n > 0 && step > 0, PNPP_ERR_ARG, "adam_step_zero: n and step must be positive");
    launch_adam({param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, grad_scale, step, nullptr, nullptr, 0.f, 1}, stream);
    PNPP_CHECK_LAUNCH("adam_step_zero");
    return PNPP_OK;
}

extern "C" int pnpp_adam_step_clip(float *param, float *grad, float *exp_avg, float *exp_avg_sq, size_t n, int step, float lr,
                                   float beta1, float beta2, float eps, float grad_scale, const double *grad_sumsq, float max_norm,
                                   int zero_grad, void *stream) {
    PNPP_REQUIRE(param && grad && exp_avg && exp_avg_sq && grad_sumsq, PNPP_ERR_ARG, "adam_step_clip: null pointer");
    PNPP_REQUIRE(n > 0 && step > 0 && max_norm > 0.f, PNPP_ERR_ARG, "adam_step_clip: n, step and max_norm must be positive");
    launch_adam({param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, grad_scale, step, nullptr, grad_sumsq, max_norm, zero_grad},
                stream);
    PNPP_CHECK_LAUNCH("adam_step_clip");
    return PNPP_OK;
}

extern "C" int pnpp_adam_step_dev(float *param, float *grad, float *exp_avg, float *exp_avg_sq, size_t n, uint64_t *step_state,
                                  float lr, float beta1, float beta2, float eps, float grad_scale, int zero_grad, void *stream) {
    PNPP_REQUIRE(param && grad && exp_avg && exp_avg_sq && step_state, PNPP_ERR_ARG, "adam_step_dev: null pointer");
    PNPP_REQUIRE(n > 0, PNPP_ERR_ARG, "adam_step_dev: n must be positive");
    launch_adam({param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, grad_scale, 0, step_state, nullptr, 0.f, zero_grad}, stream);
    PNPP_CHECK_LAUNCH("adam_step_dev");
    return PNPP_OK;
}

extern "C" int pnpp_adam_step_dev_clip(float *param, float *grad, float *exp_avg, float *exp_avg_sq, size_t n, uint64_t *step_state,
                                       float lr, float beta1, float beta2, float eps, float grad_scale, const double *grad_sumsq,
                                       float max_norm, int zero_grad, void *stream) {
    PNPP_REQUIRE(param && grad && exp_avg && exp_avg_sq && step_state && grad_sumsq, PNPP_ERR_ARG, "adam_step_dev_clip: null pointer");
    PNPP_REQUIRE(n > 0 && max_norm > 0.f, PNPP_ERR_ARG, "adam_step_dev_clip: n and max_norm must be positive");
    launch_adam({param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, grad_scale, 0, step_state, grad_sumsq, max_norm, zero_grad},
                stream);
    PNPP_CHECK_LAUNCH("adam_step_dev_clip");
    return PNPP_OK;
}

extern "C" int pnpp_sumsq(const float *x, size_t n, double *out, void *scratch, size_t scratch_bytes, void *stream) {
    PNPP_REQUIRE(x && out && scratch, PNPP_ERR_ARG, "sumsq: null pointer");
    int nb = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    if (nb < 1) nb = 1;
    PNPP_REQUIRE(scratch_bytes >= (size_t)nb * sizeof(double), PNPP_ERR_WORKSPACE, "sumsq: scratch needs %zu bytes",
                 (size_t)nb * sizeof(double));
    double *part = static_cast<double *>(scratch);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, as_stream(stream), x, n, part);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(64), 0, as_stream(stream), part, nb, out);
    PNPP_CHECK_LAUNCH("sumsq");
    return PNPP_OK;
}
