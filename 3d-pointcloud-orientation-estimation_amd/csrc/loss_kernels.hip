// loss_kernels.hip -- the stand-alone output heads and losses: von-Mises KL (value + analytic gradient in one launch), the
// multi-peak head, soft-label cross entropy, direction-vector heads with their MSE / orthogonality losses.  The one-launch step
// tails (and the matching loss, beside the tail it shares code with) are in step_tail_kernels.hip, the flat-buffer optimiser in
// optim_kernels.hip, the float64 math they share in vonmises.h.
//
// These are O(batch) scalar kernels: latency-bound, one thread per sample.
#include "kernels.h"
#include "vonmises.h"

namespace pnpp {

__global__ void __launch_bounds__(256) vm_kl_single_kernel(const float *__restrict__ mu_p, const float *__restrict__ kappa_p,
                                                           const float *__restrict__ mu_q, const float *__restrict__ kappa_q,
                                                           int n, float *__restrict__ kl, float *__restrict__ dmu,
                                                           float *__restrict__ dkappa) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v, a, b;
    kl_single_eval((double)mu_p[i], (double)kappa_p[i], (double)mu_q[i], (double)kappa_q[i], v, a, b);
    kl[i] = (float)v;
    if (dmu) dmu[i] = (float)a;
    if (dkappa) dkappa[i] = (float)b;
}

// fc3 output -> (mu, kappa) -> KL -> d/d(fc3 output); pointnet_pp_vonMises.py:36-37 fused with the loss
__global__ void __launch_bounds__(256) vm_head_kl_kernel(const float *__restrict__ o, const float *__restrict__ mu_gt,
                                                         const float *__restrict__ kappa_gt, int B, float *__restrict__ mu,
                                                         float *__restrict__ kappa, float *__restrict__ loss_vec,
                                                         float *__restrict__ d_o) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const double o0 = (double)o[2 * i], o1 = (double)o[2 * i + 1];
    const double th = tanh(o0);
    const float mu_f = (float)(th * kPi);                              // torch.tanh(out[:,0]) * np.pi
    const double sp = o1 > 20.0 ? o1 : log1p(exp(o1));                 // F.softplus (beta 1, threshold 20)
    const float kap_f = (float)sp;
    mu[i] = mu_f;
    kappa[i] = kap_f;
    if (!loss_vec) return;
    double v, a, b;
    kl_single_eval((double)mu_f, (double)kap_f, (double)mu_gt[i], (double)kappa_gt[i], v, a, b);
    loss_vec[i] = (float)v;
    if (d_o) {
        const double sig = o1 > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-o1));
        d_o[2 * i] = (float)(a * kPi * (1.0 - th * th));
        d_o[2 * i + 1] = (float)(b * sig);
    }
}

// head + KL + batch mean + gradient of the mean in ONE single-workgroup launch: the training step's loss tail
// (head, KL, mean, and the three elementwise kernels of their autograd backward) collapses into this and one multiply.
// The mean is a fixed-order fp64 tree, so it is deterministic.
__global__ void __launch_bounds__(256) vm_head_kl_mean_kernel(const float *__restrict__ o, const float *__restrict__ mu_gt,
                                                              const float *__restrict__ kappa_gt, int B, float *__restrict__ mu,
                                                              float *__restrict__ kappa, float *__restrict__ loss_vec,
                                                              float *__restrict__ loss_mean, float *__restrict__ d_o_mean) {
    __shared__ double red[256];
    __shared__ KlPieces S;
    const int lane = threadIdx.x & 63;
    const double inv_b = 1.0 / (double)B;
    double part = 0.0;
    for (int base = 0; base < B; base += 64) {
        const int i = base + lane;
        const double o0 = i < B ? (double)o[2 * i] : 0.0, o1 = i < B ? (double)o[2 * i + 1] : 0.0;
        float mu_f, kap_f, vf, g0, g1;
        if (vm_head_kl_chunk(S, i, B, o0, o1, mu_gt, kappa_gt, inv_b, mu_f, kap_f, vf, g0, g1)) {
            if (mu) mu[i] = mu_f;
            if (kappa) kappa[i] = kap_f;
            if (loss_vec) loss_vec[i] = vf;
            part += (double)vf;
            d_o_mean[2 * i] = g0;
            d_o_mean[2 * i + 1] = g1;
        }
    }
    red[threadIdx.x] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss_mean = (float)(red[0] * inv_b);
}

__global__ void __launch_bounds__(256) vm_head_bwd_kernel(const float *__restrict__ o, const float *__restrict__ dmu,
                                                          const float *__restrict__ dkappa, int B, float *__restrict__ d_o) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const double o0 = (double)o[2 * i], o1 = (double)o[2 * i + 1];
    const double th = tanh(o0);
    const double sig = o1 > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-o1));
    d_o[2 * i] = (float)((double)dmu[i] * kPi * (1.0 - th * th));
    d_o[2 * i + 1] = (float)((double)dkappa[i] * sig);
}

__global__ void __launch_bounds__(64) mvm_head_kernel(const float *__restrict__ pi_raw, const float *__restrict__ mu_raw,
                                                      const float *__restrict__ kappa_raw, int B, int K, float temp,
                                                      float kappa_max, float *__restrict__ mu, float *__restrict__ kappa,
                                                      float *__restrict__ weight) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const size_t o = (size_t)b * K;
    mvm_head_sample(pi_raw + o, mu_raw + 2 * o, kappa_raw + o, K, temp, kappa_max, mu + o, kappa + o, weight + o);
}

__global__ void __launch_bounds__(64)
mvm_head_bwd_kernel(const float *__restrict__ pi_raw, const float *__restrict__ mu_raw, const float *__restrict__ kappa_raw,
                    const float *__restrict__ weight, const float *__restrict__ dmu, const float *__restrict__ dkappa,
                    const float *__restrict__ dweight, int B, int K, float temp, float kappa_max,
                    float *__restrict__ dpi_raw, float *__restrict__ dmu_raw, float *__restrict__ dkappa_raw) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    (void)pi_raw;
    const size_t o = (size_t)b * K;
    mvm_head_bwd_sample(mu_raw + 2 * o, kappa_raw + o, weight + o, dmu + o, dkappa + o, dweight + o, K, temp, kappa_max, dpi_raw + o,
                        dmu_raw + 2 * o, dkappa_raw + o);
}

// ---- soft-label cross entropy, train_8dir_KL.py:60-68 ----------------------------------------------
__global__ void __launch_bounds__(64) soft_ce_kernel(const float *__restrict__ logits, const float *__restrict__ p, int B,
                                                     int C, float *__restrict__ loss_vec, float *__restrict__ dlogits) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float *l = logits + (size_t)b * C, *pt = p + (size_t)b * C;
    double mx = -1e300;
    for (int c = 0; c < C; ++c) mx = fmax(mx, (double)l[c]);
    double se = 0.0, sp = 0.0;
    for (int c = 0; c < C; ++c) se += exp((double)l[c] - mx), sp += (double)pt[c];
    const double lse = mx + log(se);
    double acc = 0.0;
    for (int c = 0; c < C; ++c) acc -= (double)pt[c] * ((double)l[c] - lse);
    loss_vec[b] = (float)acc;
    if (dlogits)
        for (int c = 0; c < C; ++c) dlogits[(size_t)b * C + c] = (float)(exp((double)l[c] - lse) * sp - (double)pt[c]);
}

// ---- direction-vector heads and their MSE / orthogonality losses (the other set-abstraction models) ----------------
// F.normalize(x, p=2, dim=1, eps): y = x / max(||x||, eps)            (pointnet_pp_Fwd.py:98, Pointnet_pp_xyz.py:84-85)
constexpr int VEC_CMAX = 64;
__global__ void __launch_bounds__(64) l2_normalize_kernel(const float *__restrict__ x, int M, int C, float eps,
                                                          float *__restrict__ y) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= M) return;
    const float *xr = x + (size_t)m * C;
    double ss = 0.0;
    for (int c = 0; c < C; ++c) ss += (double)xr[c] * (double)xr[c];
    const double d = fmax(sqrt(ss), (double)eps);
    for (int c = 0; c < C; ++c) y[(size_t)m * C + c] = (float)((double)xr[c] / d);
}

// dx = (dy - y (y . dy)) / ||x||  where ||x|| > eps, dy / eps otherwise (the clamp is then the constant denominator)
__global__ void __launch_bounds__(64) l2_normalize_bwd_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                              int M, int C, float eps, float *__restrict__ dx) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= M) return;
    const float *xr = x + (size_t)m * C, *gr = dy + (size_t)m * C;
    double ss = 0.0, xg = 0.0;
    for (int c = 0; c < C; ++c) ss += (double)xr[c] * (double)xr[c], xg += (double)xr[c] * (double)gr[c];
    const double nrm = sqrt(ss);
    if (nrm > (double)eps) {
        for (int c = 0; c < C; ++c) dx[(size_t)m * C + c] = (float)(((double)gr[c] - (double)xr[c] * xg / ss) / nrm);
    } else {
        for (int c = 0; c < C; ++c) dx[(size_t)m * C + c] = (float)((double)gr[c] / (double)eps);
    }
}

// nn.MSELoss(): mean over all n elements (train.py:168,183; train_multi_8dir.py:80,100); dp = 2 (p - t) / n.
// One workgroup, fixed-order float64 tree: deterministic.
__global__ void __launch_bounds__(256) mse_kernel(const float *__restrict__ p, const float *__restrict__ t, size_t n,
                                                  float *__restrict__ loss, float *__restrict__ dp) {
    __shared__ double red[256];
    double acc = 0.0;
    const double inv = 1.0 / (double)n;
    for (size_t i = threadIdx.x; i < n; i += 256) {
        const double d = (double)p[i] - (double)t[i];
        acc += d * d;
        if (dp) dp[i] = (float)(2.0 * d * inv);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(red[0] * inv);
}

// per-row mean squared error: loss_vec[b] = mean_c (p[b,c] - t[b,c])^2 -- the per-sample line of simple_pointnet_train.py:174
// (the mean of these rows is nn.MSELoss() of the batch, :153,182); dp[b,c] = 2 (p - t) / C = d loss_vec[b] / d p[b,c].
__global__ void __launch_bounds__(256) mse_rows_kernel(const float *__restrict__ p, const float *__restrict__ t, int B, int C,
                                                       float *__restrict__ loss_vec, float *__restrict__ dp) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const double inv = 1.0 / (double)C;
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
        const size_t i = (size_t)b * C + c;
        const double d = (double)p[i] - (double)t[i];
        acc += d * d;
        if (dp) dp[i] = (float)(2.0 * d * inv);
    }
    loss_vec[b] = (float)(acc * inv);
}

// orthogonality penalty of two predicted axes: mean_b (a_b . b_b)^2   (train.py:184-185)
__global__ void __launch_bounds__(256) orth_loss_kernel(const float *__restrict__ a, const float *__restrict__ b, int B, int C,
                                                        float *__restrict__ loss, float *__restrict__ da,
                                                        float *__restrict__ db) {
    __shared__ double red[256];
    double acc = 0.0;
    const double inv = 1.0 / (double)B;
    for (int m = threadIdx.x; m < B; m += 256) {
        double dot = 0.0;
        for (int c = 0; c < C; ++c) dot += (double)a[(size_t)m * C + c] * (double)b[(size_t)m * C + c];
        acc += dot * dot;
        if (da && db)
            for (int c = 0; c < C; ++c) {
                da[(size_t)m * C + c] = (float)(2.0 * dot * inv * (double)b[(size_t)m * C + c]);
                db[(size_t)m * C + c] = (float)(2.0 * dot * inv * (double)a[(size_t)m * C + c]);
            }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(red[0] * inv);
}

// proj_probs (train_multi_8dir.py:41-44): v = normalize(vec); sims = clamp(v D^T, min=0); p = sims / clamp(sum sims, 1e-8)
constexpr int PROJ_DMAX = 16;
__global__ void __launch_bounds__(64) proj_probs_kernel(const float *__restrict__ vec, const float *__restrict__ dirs, int B,
                                                        int D, float *__restrict__ probs) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= B) return;
    const double x0 = vec[3 * m], x1 = vec[3 * m + 1], x2 = vec[3 * m + 2];
    const double d = fmax(sqrt(x0 * x0 + x1 * x1 + x2 * x2), 1e-12);
    const float v0 = (float)(x0 / d), v1 = (float)(x1 / d), v2 = (float)(x2 / d);  // F.normalize's float32 result
    double sims[PROJ_DMAX], sum = 0.0;
    for (int j = 0; j < D; ++j) {
        const double dot = (double)v0 * (double)dirs[3 * j] + (double)v1 * (double)dirs[3 * j + 1] + (double)v2 * (double)dirs[3 * j + 2];
        sims[j] = fmax(dot, 0.0);
        sum += sims[j];
    }
    const double s = fmax(sum, 1e-8);
    for (int j = 0; j < D; ++j) probs[(size_t)m * D + j] = (float)(sims[j] / s);
}

__global__ void __launch_bounds__(64) proj_probs_bwd_kernel(const float *__restrict__ vec, const float *__restrict__ dirs,
                                                            const float *__restrict__ dprobs, int B, int D,
                                                            float *__restrict__ dvec) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= B) return;
    const double x0 = vec[3 * m], x1 = vec[3 * m + 1], x2 = vec[3 * m + 2];
    const double ss = x0 * x0 + x1 * x1 + x2 * x2, nrm = sqrt(ss), d = fmax(nrm, 1e-12);
    const double v0 = x0 / d, v1 = x1 / d, v2 = x2 / d;
    double dots[PROJ_DMAX], sum = 0.0, gs = 0.0;
    for (int j = 0; j < D; ++j) {
        dots[j] = v0 * (double)dirs[3 * j] + v1 * (double)dirs[3 * j + 1] + v2 * (double)dirs[3 * j + 2];
        const double sj = fmax(dots[j], 0.0);
        sum += sj;
        gs += (double)dprobs[(size_t)m * D + j] * sj;
    }
    const double s = fmax(sum, 1e-8);
    const double back = sum >= 1e-8 ? gs / (s * s) : 0.0;  // the clamped denominator is a constant below 1e-8
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;                   // gradient w.r.t. the unit vector
    for (int j = 0; j < D; ++j) {
        if (!(dots[j] >= 0.0)) continue;                    // clamp(min=0) passes the gradient where its input >= 0
        const double gj = (double)dprobs[(size_t)m * D + j] / s - back;
        g0 += gj * (double)dirs[3 * j], g1 += gj * (double)dirs[3 * j + 1], g2 += gj * (double)dirs[3 * j + 2];
    }
    if (nrm > 1e-12) {
        const double vg = v0 * g0 + v1 * g1 + v2 * g2;
        dvec[3 * m] = (float)((g0 - v0 * vg) / nrm), dvec[3 * m + 1] = (float)((g1 - v1 * vg) / nrm);
        dvec[3 * m + 2] = (float)((g2 - v2 * vg) / nrm);
    } else {
        dvec[3 * m] = (float)(g0 / 1e-12), dvec[3 * m + 1] = (float)(g1 / 1e-12), dvec[3 * m + 2] = (float)(g2 / 1e-12);
    }
}

}  // namespace pnpp

using namespace pnpp;

extern "C" int pnpp_vm_kl_single(const float *mu_p, const float *kappa_p, const float *mu_q, const float *kappa_q, int n,
                                 float *kl, float *dmu, float *dkappa, void *stream) {
    PNPP_REQUIRE(mu_p && kappa_p && mu_q && kappa_q && kl, PNPP_ERR_ARG, "vm_kl_single: null pointer");
    PNPP_REQUIRE(n > 0, PNPP_ERR_ARG, "vm_kl_single: n must be positive");
    hipLaunchKernelGGL(vm_kl_single_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), mu_p, kappa_p, mu_q, kappa_q,
                       n, kl, dmu, dkappa);
    PNPP_CHECK_LAUNCH("vm_kl_single");
    return PNPP_OK;
}

extern "C" int pnpp_vm_head_kl(const float *o, const float *mu_gt, const float *kappa_gt, int B, float *mu, float *kappa,
                               float *loss_vec, float *d_o, void *stream) {
    PNPP_REQUIRE(o && mu && kappa, PNPP_ERR_ARG, "vm_head_kl: null pointer");
    PNPP_REQUIRE(!loss_vec || (mu_gt && kappa_gt), PNPP_ERR_ARG, "vm_head_kl: loss requested without ground truth");
    PNPP_REQUIRE(B > 0, PNPP_ERR_ARG, "vm_head_kl: B must be positive");
    hipLaunchKernelGGL(vm_head_kl_kernel, dim3(cdiv(B, 256)), dim3(256), 0, as_stream(stream), o, mu_gt, kappa_gt, B, mu, kappa,
                       loss_vec, d_o);
    PNPP_CHECK_LAUNCH("vm_head_kl");
    return PNPP_OK;
}

extern "C" int pnpp_vm_head_kl_mean(const float *o, const float *mu_gt, const float *kappa_gt, int B, float *mu, float *kappa,
                                    float *loss_vec, float *loss_mean, float *d_o_mean, void *stream) {
    PNPP_REQUIRE(o && mu_gt && kappa_gt && loss_mean && d_o_mean, PNPP_ERR_ARG, "vm_head_kl_mean: null pointer");
    PNPP_REQUIRE(B > 0, PNPP_ERR_ARG, "vm_head_kl_mean: B must be positive");
    hipLaunchKernelGGL(vm_head_kl_mean_kernel, dim3(1), dim3(256), 0, as_stream(stream), o, mu_gt, kappa_gt, B, mu, kappa,
                       loss_vec, loss_mean, d_o_mean);
    PNPP_CHECK_LAUNCH("vm_head_kl_mean");
    return PNPP_OK;
}

extern "C" int pnpp_vm_head_bwd(const float *o, const float *dmu, const float *dkappa, int B, float *d_o, void *stream) {
    PNPP_REQUIRE(o && dmu && dkappa && d_o, PNPP_ERR_ARG, "vm_head_bwd: null pointer");
    PNPP_REQUIRE(B > 0, PNPP_ERR_ARG, "vm_head_bwd: B must be positive");
    hipLaunchKernelGGL(vm_head_bwd_kernel, dim3(cdiv(B, 256)), dim3(256), 0, as_stream(stream), o, dmu, dkappa, B, d_o);
    PNPP_CHECK_LAUNCH("vm_head_bwd");
    return PNPP_OK;
}

extern "C" int pnpp_mvm_head(const float *pi_raw, const float *mu_raw, const float *kappa_raw, int B, int K, float temp,
                             float kappa_max, float *mu, float *kappa, float *weight, void *stream) {
    PNPP_REQUIRE(pi_raw && mu_raw && kappa_raw && mu && kappa && weight, PNPP_ERR_ARG, "mvm_head: null pointer");
    PNPP_REQUIRE(B > 0 && K > 0, PNPP_ERR_ARG, "mvm_head: non-positive size");
    hipLaunchKernelGGL(mvm_head_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), pi_raw, mu_raw, kappa_raw, B, K, temp,
                       kappa_max, mu, kappa, weight);
    PNPP_CHECK_LAUNCH("mvm_head");
    return PNPP_OK;
}

extern "C" int pnpp_mvm_head_bwd(const float *pi_raw, const float *mu_raw, const float *kappa_raw, const float *weight,
                                 const float *dmu, const float *dkappa, const float *dweight, int B, int K, float temp,
                                 float kappa_max, float *dpi_raw, float *dmu_raw, float *dkappa_raw, void *stream) {
    PNPP_REQUIRE(pi_raw && mu_raw && kappa_raw && weight && dmu && dkappa && dweight && dpi_raw && dmu_raw && dkappa_raw,
                 PNPP_ERR_ARG, "mvm_head_bwd: null pointer");
    PNPP_REQUIRE(B > 0 && K > 0, PNPP_ERR_ARG, "mvm_head_bwd: non-positive size");
    hipLaunchKernelGGL(mvm_head_bwd_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), pi_raw, mu_raw, kappa_raw, weight,
                       dmu, dkappa, dweight, B, K, temp, kappa_max, dpi_raw, dmu_raw, dkappa_raw);
    PNPP_CHECK_LAUNCH("mvm_head_bwd");
    return PNPP_OK;
}

extern "C" int pnpp_l2_normalize(const float *x, int M, int C, float eps, float *y, void *stream) {
    PNPP_REQUIRE(x && y, PNPP_ERR_ARG, "l2_normalize: null pointer");
    PNPP_REQUIRE(M > 0 && C > 0 && C <= VEC_CMAX, PNPP_ERR_ARG, "l2_normalize: M=%d C=%d (C <= %d)", M, C, VEC_CMAX);
    hipLaunchKernelGGL(l2_normalize_kernel, dim3(cdiv(M, 64)), dim3(64), 0, as_stream(stream), x, M, C, eps, y);
    PNPP_CHECK_LAUNCH("l2_normalize");
    return PNPP_OK;
}

extern "C" int pnpp_l2_normalize_bwd(const float *x, const float *dy, int M, int C, float eps, float *dx, void *stream) {
    PNPP_REQUIRE(x && dy && dx, PNPP_ERR_ARG, "l2_normalize_bwd: null pointer");
    PNPP_REQUIRE(M > 0 && C > 0 && C <= VEC_CMAX, PNPP_ERR_ARG, "l2_normalize_bwd: M=%d C=%d (C <= %d)", M, C, VEC_CMAX);
    hipLaunchKernelGGL(l2_normalize_bwd_kernel, dim3(cdiv(M, 64)), dim3(64), 0, as_stream(stream), x, dy, M, C, eps, dx);
    PNPP_CHECK_LAUNCH("l2_normalize_bwd");
    return PNPP_OK;
}

extern "C" int pnpp_mse(const float *p, const float *t, size_t n, float *loss, float *dp, void *stream) {
    PNPP_REQUIRE(p && t && loss, PNPP_ERR_ARG, "mse: null pointer");
    PNPP_REQUIRE(n > 0, PNPP_ERR_ARG, "mse: empty input");
    hipLaunchKernelGGL(mse_kernel, dim3(1), dim3(256), 0, as_stream(stream), p, t, n, loss, dp);
    PNPP_CHECK_LAUNCH("mse");
    return PNPP_OK;
}

extern "C" int pnpp_mse_rows(const float *p, const float *t, int B, int C, float *loss_vec, float *dp, void *stream) {
    PNPP_REQUIRE(p && t && loss_vec, PNPP_ERR_ARG, "mse_rows: null pointer");
    PNPP_REQUIRE(B > 0 && C > 0, PNPP_ERR_ARG, "mse_rows: B=%d C=%d", B, C);
    hipLaunchKernelGGL(mse_rows_kernel, dim3(cdiv(B, 256)), dim3(256), 0, as_stream(stream), p, t, B, C, loss_vec, dp);
    PNPP_CHECK_LAUNCH("mse_rows");
    return PNPP_OK;
}

extern "C" int pnpp_orth_loss(const float *a, const float *b, int B, int C, float *loss, float *da, float *db, void *stream) {
    PNPP_REQUIRE(a && b && loss, PNPP_ERR_ARG, "orth_loss: null pointer");
    PNPP_REQUIRE((da == nullptr) == (db == nullptr), PNPP_ERR_ARG, "orth_loss: pass both gradient outputs or neither");
    PNPP_REQUIRE(B > 0 && C > 0, PNPP_ERR_ARG, "orth_loss: non-positive size");
    hipLaunchKernelGGL(orth_loss_kernel, dim3(1), dim3(256), 0, as_stream(stream), a, b, B, C, loss, da, db);
    PNPP_CHECK_LAUNCH("orth_loss");
    return PNPP_OK;
}

extern "C" int pnpp_proj_probs(const float *vec, const float *dirs, int B, int D, float *probs, void *stream) {
    PNPP_REQUIRE(vec && dirs && probs, PNPP_ERR_ARG, "proj_probs: null pointer");
    PNPP_REQUIRE(B > 0 && D > 0 && D <= PROJ_DMAX, PNPP_ERR_ARG, "proj_probs: B=%d D=%d (D <= %d)", B, D, PROJ_DMAX);
    hipLaunchKernelGGL(proj_probs_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), vec, dirs, B, D, probs);
    PNPP_CHECK_LAUNCH("proj_probs");
    return PNPP_OK;
}

extern "C" int pnpp_proj_probs_bwd(const float *vec, const float *dirs, const float *dprobs, int B, int D, float *dvec,
                                   void *stream) {
    PNPP_REQUIRE(vec && dirs && dprobs && dvec, PNPP_ERR_ARG, "proj_probs_bwd: null pointer");
    PNPP_REQUIRE(B > 0 && D > 0 && D <= PROJ_DMAX, PNPP_ERR_ARG, "proj_probs_bwd: B=%d D=%d (D <= %d)", B, D, PROJ_DMAX);
    hipLaunchKernelGGL(proj_probs_bwd_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), vec, dirs, dprobs, B, D, dvec);
    PNPP_CHECK_LAUNCH("proj_probs_bwd");
    return PNPP_OK;
}

extern "C" int pnpp_soft_ce(const float *logits, const float *p, int B, int C, float *loss_vec, float *dlogits, void *stream) {
    PNPP_REQUIRE(logits && p && loss_vec, PNPP_ERR_ARG, "soft_ce: null pointer");
    PNPP_REQUIRE(B > 0 && C > 0, PNPP_ERR_ARG, "soft_ce: non-positive size");
    hipLaunchKernelGGL(soft_ce_kernel, dim3(cdiv(B, 64)), dim3(64), 0, as_stream(stream), logits, p, B, C, loss_vec, dlogits);
    PNPP_CHECK_LAUNCH("soft_ce");
    return PNPP_OK;
}
