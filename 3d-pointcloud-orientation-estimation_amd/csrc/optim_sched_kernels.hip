// optim_sched_kernels.hip -- the flat-buffer optimiser with what a training loop wants beyond constant-rate Adam, still one launch:
// parameter groups (a learning-rate multiplier and a weight decay each), decoupled (AdamW) or L2 weight decay, a learning-rate schedule
// evaluated on the device from the step count kept there (a captured launch applies its own rate at every replay), and an exponential
// moving average of the weights.  optim_kernels.hip's entries are untouched; with every addition off this kernel's results equal
// adam_dev_kernel's bit for bit (tests/test_gpu_optim_sched.py holds the two together).
//
// This file is compiled with -ffp-contract=off: every float32 operation below is written out, the two fused multiply-adds included, so
// that the roundings can be counted from the text.
#include "kernels.h"
#include "lr_schedule.h"

namespace pnpp {

// optim_kernels.hip's clip_coef, restated (that file stays as it is): min(1, max_norm / (norm + 1e-6)) with norm = sqrt(sumsq) * gscale
__device__ __forceinline__ float sched_clip_coef(const double *__restrict__ sumsq, float gscale, float max_norm) {
    if (!sumsq) return 1.f;
    const float norm = (float)(sqrt(sumsq[0]) * (double)gscale);
    return fminf(1.f, max_norm / (norm + 1e-6f));
}

// what thread 0 of a workgroup works out in float64 for all of them
struct SchedCoefs {
    float step[PNPP_OPTIM_MAX_GROUPS];    // (float)(lr_g / bc1),  lr_g = (lr f) mult_g
    float decay[PNPP_OPTIM_MAX_GROUPS];   // (float)(1 - lr_g wd_g)
    float wd[PNPP_OPTIM_MAX_GROUPS];
    float inv_sqrt_bc2;                   // (float)(1 / sqrt(bc2))
    unsigned long long step_no;
    double rate;                          // lr f
};

struct ElemCoefs {
    float gscale, b1, omb1, b2, omb2, eps, inv_sqrt_bc2, ema_d, ema_omd;
    int decoupled, ema_on;
};

// An element's group: the number of ends at or below its index.  The host pads end[] with ~0 beyond n_groups, so all eight compare.
__device__ __forceinline__ int group_of(const pnpp_optim_desc &d, size_t i) {
    int k = 0;
#pragma unroll
    for (int j = 0; j < PNPP_OPTIM_MAX_GROUPS - 1; ++j) k += (d.end[j] <= (uint64_t)i) ? 1 : 0;
    return k;
}

// One element, float32, one rounding per operation in this order (adam_dev_kernel's operations where both have them):
//   gi = g * gscale                                   gscale = grad_scale * clip coefficient, once per thread
//   L2 mode, wd_g != 0:   gi = gi + (wd_g * p)        two roundings
//   mi = fma(1 - b1, gi, b1 * m)                      b1 * m rounded, then one fused multiply-add
//   vi = b2 * v + ((1 - b2) * gi) * gi                four roundings
//   denom = fma(sqrt(vi), inv_sqrt_bc2, eps)          sqrt correctly rounded, then one fused multiply-add
//   upd = (step_g * mi) / denom                       two roundings
//   decoupled mode:       p = p * decay_g             one rounding (decay_g is 1 where wd_g or lr_g is 0: exact)
//   p = p - upd
//   average on:           e = (d * e) + ((1 - d) * p) three roundings, (1 - d) rounded once from float64 on the host
__device__ __forceinline__ void update_one(float &p, float g, float &m, float &v, float *e, const ElemCoefs &c, float step, float decay,
                                           float wd) {
    float gi = g * c.gscale;
    if (!c.decoupled && wd != 0.f) gi = gi + wd * p;
    const float mi = __builtin_fmaf(c.omb1, gi, c.b1 * m);
    const float vi = c.b2 * v + (c.omb2 * gi) * gi;
    const float denom = __builtin_fmaf(sqrtf(vi), c.inv_sqrt_bc2, c.eps);
    const float upd = (step * mi) / denom;
    const float pd = c.decoupled ? p * decay : p;
    m = mi;
    v = vi;
    p = pd - upd;
    if (c.ema_on) *e = c.ema_d * *e + c.ema_omd * p;
}

// W = 1: one element per lane and trip, as adam_dev_kernel.  W = 4: 16 bytes per lane and buffer (all buffers 16-byte aligned), quads
// that straddle a group boundary look their coefficients up per element, the n % 4 elements past the last quad go to the first lanes of
// the grid.  state[0], state[1]: adam_dev_kernel's count and ticket, same protocol; the last workgroup also leaves the rate in state[2].
template <int W>
__global__ void __launch_bounds__(256) adamw_sched_kernel(const pnpp_optim_desc d, float *__restrict__ p, float *__restrict__ g,
                                                          float *__restrict__ m, float *__restrict__ v, float *__restrict__ ema, size_t n,
                                                          unsigned long long *__restrict__ state, const double *__restrict__ sumsq,
                                                          float ema_omd) {
    __shared__ SchedCoefs S;
    if (threadIdx.x == 0) {
        const unsigned long long s = state[0], t = s + 1ull;
        const double bc1 = 1.0 - pow((double)d.beta1, (double)t), bc2 = 1.0 - pow((double)d.beta2, (double)t);
        const double rate = (double)d.lr * lr_schedule_factor(d, s);
#pragma unroll
        for (int j = 0; j < PNPP_OPTIM_MAX_GROUPS; ++j) {
            const double lr_g = rate * (double)d.lr_mult[j];
            S.step[j] = (float)(lr_g / bc1);
            S.decay[j] = (float)(1.0 - lr_g * (double)d.weight_decay[j]);
            S.wd[j] = d.weight_decay[j];
        }
        S.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        S.step_no = t;
        S.rate = rate;
    }
    __syncthreads();
    ElemCoefs c;
    c.gscale = d.grad_scale * sched_clip_coef(sumsq, d.grad_scale, d.max_norm);
    c.b1 = d.beta1, c.omb1 = 1.f - d.beta1, c.b2 = d.beta2, c.omb2 = 1.f - d.beta2, c.eps = d.eps;
    c.inv_sqrt_bc2 = S.inv_sqrt_bc2;
    c.ema_d = d.ema_decay, c.ema_omd = ema_omd, c.ema_on = ema != nullptr, c.decoupled = d.decoupled;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (W == 1) {
        for (size_t i = tid; i < n; i += stride) {
            const int k = group_of(d, i);
            float pi = p[i], mi = m[i], vi = v[i];
            update_one(pi, g[i], mi, vi, ema ? ema + i : nullptr, c, S.step[k], S.decay[k], S.wd[k]);
            m[i] = mi;
            v[i] = vi;
            p[i] = pi;
            if (d.zero_grad) g[i] = 0.f;
        }
    } else {
        const size_t nq = n / 4;
        for (size_t q = tid; q < nq; q += stride) {
            const size_t i = q * 4;
            float4 p4 = reinterpret_cast<float4 *>(p)[q], m4 = reinterpret_cast<float4 *>(m)[q], v4 = reinterpret_cast<float4 *>(v)[q];
            const float4 g4 = reinterpret_cast<const float4 *>(g)[q];
            float4 e4 = ema ? reinterpret_cast<float4 *>(ema)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            const int k0 = group_of(d, i), k3 = group_of(d, i + 3);
            const int k1 = k0 == k3 ? k0 : group_of(d, i + 1), k2 = k0 == k3 ? k0 : group_of(d, i + 2);
            update_one(p4.x, g4.x, m4.x, v4.x, &e4.x, c, S.step[k0], S.decay[k0], S.wd[k0]);
            update_one(p4.y, g4.y, m4.y, v4.y, &e4.y, c, S.step[k1], S.decay[k1], S.wd[k1]);
            update_one(p4.z, g4.z, m4.z, v4.z, &e4.z, c, S.step[k2], S.decay[k2], S.wd[k2]);
            update_one(p4.w, g4.w, m4.w, v4.w, &e4.w, c, S.step[k3], S.decay[k3], S.wd[k3]);
            reinterpret_cast<float4 *>(m)[q] = m4;
            reinterpret_cast<float4 *>(v)[q] = v4;
            reinterpret_cast<float4 *>(p)[q] = p4;
            if (ema) reinterpret_cast<float4 *>(ema)[q] = e4;
            if (d.zero_grad) reinterpret_cast<float4 *>(g)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const size_t i = nq * 4 + tid;   // the n % 4 elements past the last quad
        if (tid < 4 && i < n) {
            const int k = group_of(d, i);
            float pi = p[i], mi = m[i], vi = v[i];
            update_one(pi, g[i], mi, vi, ema ? ema + i : nullptr, c, S.step[k], S.decay[k], S.wd[k]);
            m[i] = mi;
            v[i] = vi;
            p[i] = pi;
            if (d.zero_grad) g[i] = 0.f;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = atomicAdd(&state[1], 1ull);
        if (t == (unsigned long long)gridDim.x - 1ull) {
            state[1] = 0ull;
            state[2] = (unsigned long long)__double_as_longlong(S.rate);
            state[0] = S.step_no;
        }
    }
}

}  // namespace pnpp

using namespace pnpp;

static bool unit_interval(double x) { return x >= 0.0 && x <= 1.0; }   // false for NaN

// The schedule fields of a descriptor, for both entries (who: the entry's name in the message)
static int check_schedule(const pnpp_optim_desc *d, const char *who) {
    PNPP_REQUIRE(d->sched_kind == PNPP_SCHED_CONSTANT || d->sched_kind == PNPP_SCHED_COSINE || d->sched_kind == PNPP_SCHED_STEP, PNPP_ERR_ARG,
                 "%s: unknown sched_kind %d", who, d->sched_kind);
    PNPP_REQUIRE(unit_interval(d->start_factor) && unit_interval(d->min_factor), PNPP_ERR_ARG,
                 "%s: start_factor and min_factor must lie in [0, 1]", who);
    PNPP_REQUIRE(d->sched_kind != PNPP_SCHED_COSINE || d->total > d->warmup, PNPP_ERR_ARG, "%s: a cosine schedule needs total > warmup", who);
    PNPP_REQUIRE(d->sched_kind != PNPP_SCHED_STEP || (d->every > 0 && d->gamma > 0.0 && d->gamma <= 1.0), PNPP_ERR_ARG,
                 "%s: a step schedule needs every > 0 and gamma in (0, 1]", who);
    return PNPP_OK;
}

extern "C" int pnpp_lr_factor(const pnpp_optim_desc *d, uint64_t steps_taken, double *factor) {
    PNPP_REQUIRE(d && factor, PNPP_ERR_ARG, "lr_factor: null pointer");
    PNPP_TRY(check_schedule(d, "lr_factor"));
    *factor = lr_schedule_factor(*d, steps_taken);
    return PNPP_OK;
}

extern "C" int pnpp_adamw_step(const pnpp_optim_desc *d, float *param, float *grad, float *exp_avg, float *exp_avg_sq, float *ema, size_t n,
                               uint64_t *step_state, const double *grad_sumsq, void *stream) {
    PNPP_REQUIRE(d && param && grad && exp_avg && exp_avg_sq && step_state, PNPP_ERR_ARG, "adamw_step: null pointer");
    PNPP_REQUIRE(n > 0, PNPP_ERR_ARG, "adamw_step: n must be positive");
    PNPP_REQUIRE(d->n_groups >= 1 && d->n_groups <= PNPP_OPTIM_MAX_GROUPS, PNPP_ERR_ARG, "adamw_step: n_groups must be 1 .. %d",
                 PNPP_OPTIM_MAX_GROUPS);
    for (int j = 0; j < d->n_groups; ++j) {
        PNPP_REQUIRE(d->end[j] > (j ? d->end[j - 1] : 0), PNPP_ERR_ARG, "adamw_step: end[] must be strictly increasing from above 0");
        PNPP_REQUIRE(d->lr_mult[j] >= 0.f && isfinite(d->lr_mult[j]) && d->weight_decay[j] >= 0.f && isfinite(d->weight_decay[j]),
                     PNPP_ERR_ARG, "adamw_step: lr_mult and weight_decay must be finite and not negative");
    }
    PNPP_REQUIRE(d->end[d->n_groups - 1] == (uint64_t)n, PNPP_ERR_ARG, "adamw_step: the last end must equal n");
    PNPP_REQUIRE(d->ema_decay >= 0.f && d->ema_decay < 1.f, PNPP_ERR_ARG, "adamw_step: ema_decay must lie in [0, 1)");
    PNPP_REQUIRE((d->ema_decay > 0.f) == (ema != nullptr), PNPP_ERR_ARG, "adamw_step: ema must be given exactly when ema_decay > 0");
    PNPP_REQUIRE(d->max_norm >= 0.f, PNPP_ERR_ARG, "adamw_step: max_norm must not be negative");
    PNPP_REQUIRE(d->max_norm == 0.f || grad_sumsq, PNPP_ERR_ARG, "adamw_step: clipping (max_norm > 0) needs grad_sumsq");
    PNPP_TRY(check_schedule(d, "adamw_step"));

    pnpp_optim_desc k = *d;   // what the kernel reads: ends past the last group never compare below an index, their coefficients are inert
    for (int j = d->n_groups; j < PNPP_OPTIM_MAX_GROUPS; ++j) k.end[j] = ~0ull, k.lr_mult[j] = 0.f, k.weight_decay[j] = 0.f;
    k.decoupled = d->decoupled != 0;
    const float ema_omd = (float)(1.0 - (double)d->ema_decay);
    const double *sumsq = d->max_norm > 0.f ? grad_sumsq : nullptr;
    auto *state = reinterpret_cast<unsigned long long *>(step_state);
    const auto misaligned = [](const void *q) { return q && (reinterpret_cast<uintptr_t>(q) & 15) != 0; };
    const bool wide = !(misaligned(param) || misaligned(grad) || misaligned(exp_avg) || misaligned(exp_avg_sq) || misaligned(ema));
    const size_t work = wide ? (n / 4 > 0 ? n / 4 : 1) : n;
    const int grid = (int)((work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048);
    const auto kernel = wide ? adamw_sched_kernel<4> : adamw_sched_kernel<1>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, as_stream(stream), k, param, grad, exp_avg, exp_avg_sq, ema, n, state, sumsq, ema_omd);
    PNPP_CHECK_LAUNCH("adamw_step");
    return PNPP_OK;
}
