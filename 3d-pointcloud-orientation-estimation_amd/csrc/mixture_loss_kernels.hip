// mixture_loss_kernels.hip -- the mixture KL of the multi-peak model on the decode grid: KL(ground truth || prediction) of two
// von-Mises mixtures by the periodic rectangle rule, value and the three analytic gradients from one pass.
//
//   q(t) = sum_{j < K_gt} v_j vM(t; nu_j, lambda_j)      v normalised by the sum of its positive entries
//   p(t) = sum_{i < max_K} w_i vM(t; mu_i, kappa_i)      every predicted component, weights as given
//   loss = (2 pi / G) sum_g q(t_g) (log q(t_g) - log p(t_g)),   t_g = 2 pi g / G
//
// Unlike match_loss (vonmises.h) it charges EVERY predicted component for the mass it carries, and its gradient with respect to mu is
// not zero at the head's zero initialisation once the components start at distinct angles.  The integrand is analytic and periodic, so
// the rectangle rule converges geometrically: at G = 359 it equals the closed-form KL of two von-Mises densities to 6e-14 for every
// kappa <= 500.  Everything is float64 in the log domain (log vM = kappa (cos - 1) - log(2 pi i0e(kappa)), log-sum-exp over the
// components) and rounded once to float32 on the way out.
//
// Built with the flags of loss_kernels.hip: the head form runs mvm_head_sample / mvm_head_bwd_sample of vonmises.h around the same
// grid pass and is compared bit for bit with pnpp_mvm_head -> pnpp_mvm_grid_kl -> pnpp_mvm_head_bwd.
#include "kernels.h"
#include "vonmises.h"

namespace pnpp {

constexpr int GKL_GMAX = 1024;   // grid points of a sample (num - 1), as pnpp_mvm_decode
constexpr double kGklKappaMax = 500.0;

template <int MK>
struct GridKlShared {
    // prediction: lnorm = -log(2 pi i0e(kappa)), lw = log w (-inf: the component is skipped in log p), A = I1 / I0, pass = the clamp's
    // derivative; ground truth: lv = log(v / sum v) - log(2 pi i0e(lambda)) (-inf: skipped)
    double mu[MK], kap[MK], lnorm[MK], lw[MK], w[MK], A[MK], pass[MK];
    double nu[MK], lam[MK], lv[MK];
    double red[4][1 + 3 * MK];
    float hmu[MK], hkap[MK], hw[MK];   // the prediction as float32: read from memory, or the head's outputs
    float gmu[MK], gkap[MK], gw[MK];   // d loss / d (mu, kappa, weight), float32, for the head's backward
    int live;                          // 0: K_gt <= 0 or no positive ground-truth weight -> loss 0, zero gradients
};

__device__ __forceinline__ double gkl_clamp(double k, double &pass) {
    pass = (k >= 0.0 && k <= kGklKappaMax) ? 1.0 : 0.0;
    return k < 0.0 ? 0.0 : k > kGklKappaMax ? kGklKappaMax : k;
}

// One workgroup of four waves per sample.  (0, HEAD) one lane runs the head into LDS; (1) the first K_gt + max_K threads fill the
// component tables; (2) each thread walks the grid points tid, tid + 256, ... with 1 + 3 max_K float64 partial sums in registers;
// (3) wave butterflies, then the four waves' sums in a fixed order: no atomics, two calls are bit-identical; (4, HEAD) one lane runs the
// head's backward.  MK: the compile-time bound of max_K; every loop over components runs to MK under an `i < K` test, so that no
// register array is indexed by a run-time value (vonmises.h: match_assign_sample).
template <int MK, bool HEAD>
__global__ void __launch_bounds__(256)
mvm_grid_kl_kernel(const float *__restrict__ in0, const float *__restrict__ in1, const float *__restrict__ in2,
                   const float *__restrict__ vm_gt, const int32_t *__restrict__ K_gt, int K, int G, float temp, float kappa_max,
                   float *__restrict__ loss_vec, float *__restrict__ d0, float *__restrict__ d1, float *__restrict__ d2,
                   float *__restrict__ o_mu, float *__restrict__ o_kappa, float *__restrict__ o_weight) {
    __shared__ GridKlShared<MK> S;
    constexpr int NS = 1 + 3 * MK;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t o = (size_t)b * K;
    const bool want = d0 != nullptr;
    int Kg = K_gt[b];
    Kg = Kg < 0 ? 0 : Kg > K ? K : Kg;

    // ---- (0) the prediction as float32 ----
    if (HEAD) {   // in0, in1, in2 = pi_raw (B,K), mu_raw (B,2K), kappa_raw (B,K)
        if (tid == 0) {
            mvm_head_sample(in0 + o, in1 + 2 * o, in2 + o, K, temp, kappa_max, S.hmu, S.hkap, S.hw);
            if (o_mu)
                for (int k = 0; k < K; ++k) o_mu[o + k] = S.hmu[k], o_kappa[o + k] = S.hkap[k], o_weight[o + k] = S.hw[k];
        }
    } else if (tid < K) {   // in0, in1, in2 = mu, kappa, weight (B,K)
        S.hmu[tid] = in0[o + tid], S.hkap[tid] = in1[o + tid], S.hw[tid] = in2[o + tid];
    }
    __syncthreads();

    // ---- (1) the component tables: a Bessel series or two per thread ----
    if (tid < K) {
        double pass;
        const double kp = gkl_clamp((double)S.hkap[tid], pass), w = (double)S.hw[tid];
        const double e0 = i0e(kp);
        S.mu[tid] = (double)S.hmu[tid], S.kap[tid] = kp, S.pass[tid] = pass;
        S.lnorm[tid] = -log(2.0 * kPi * e0);
        S.A[tid] = i1e(kp) / e0;
        S.w[tid] = w > 0.0 ? w : 0.0;
        S.lw[tid] = w > 0.0 ? log(w) : -__builtin_inf();
    } else if (tid < K + Kg) {
        const int j = tid - K;
        const float *row = vm_gt + (o + j) * 3;
        double sv = 0.0;
        for (int l = 0; l < Kg; ++l) {
            const double v = (double)vm_gt[(o + l) * 3 + 2];
            if (v > 0.0) sv += v;
        }
        double pass;
        const double lam = gkl_clamp((double)row[1], pass), v = (double)row[2];
        S.nu[j] = (double)row[0], S.lam[j] = lam;
        S.lv[j] = v > 0.0 ? log(v / sv) - log(2.0 * kPi * i0e(lam)) : -__builtin_inf();
        if (j == 0) S.live = sv > 0.0 ? 1 : 0;
    }
    if (Kg == 0 && tid == 0) S.live = 0;
    __syncthreads();
    const bool live = S.live != 0;

    // ---- (2) the grid ----
    double acc[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) acc[n] = 0.0;
    if (live) {
        for (int g = tid; g < G; g += 256) {
            const double th = (double)g * (2.0 * kPi) / (double)G;
            double aq[MK], mq = -__builtin_inf();
#pragma unroll
            for (int j = 0; j < MK; ++j)
                if (j < Kg) {
                    aq[j] = S.lam[j] * (cos(th - S.nu[j]) - 1.0) + S.lv[j];
                    mq = fmax(mq, aq[j]);
                }
            double sq = 0.0;
#pragma unroll
            for (int j = 0; j < MK; ++j)
                if (j < Kg) sq += exp(aq[j] - mq);
            const double lq = mq + log(sq);

            double e[MK], cs[MK], sn[MK], mp = -__builtin_inf();
#pragma unroll
            for (int i = 0; i < MK; ++i)
                if (i < K) {
                    const double d = th - S.mu[i];
                    cs[i] = cos(d), sn[i] = sin(d);
                    e[i] = S.kap[i] * (cs[i] - 1.0) + S.lnorm[i];
                    mp = fmax(mp, e[i] + S.lw[i]);
                }
            double sp = 0.0;
#pragma unroll
            for (int i = 0; i < MK; ++i)
                if (i < K) sp += exp(e[i] + S.lw[i] - mp);
            const double lp = mp + log(sp);
            acc[0] += exp(lq) * (lq - lp);
            if (want) {
#pragma unroll
                for (int i = 0; i < MK; ++i)
                    if (i < K) {
                        const double qv = exp(lq + e[i] - lp);   // q vM_i / p
                        const double qr = S.w[i] * qv;           // q r_i
                        acc[1 + i] += qr * sn[i];
                        acc[1 + MK + i] += qr * (cs[i] - S.A[i]);
                        acc[1 + 2 * MK + i] += qv;
                    }
            }
        }
    }

    // ---- (3) one order of summation: butterfly inside each wave, then ((w0 + w1) + (w2 + w3)) ----
#pragma unroll
    for (int n = 0; n < NS; ++n) {
        if (n == 0 || want) {
            double v = acc[n];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_f64(v, m);
            if (lane == 0) S.red[wave][n] = v;
        }
    }
    __syncthreads();
    const double c = 2.0 * kPi / (double)G;
    if (tid < NS && (tid == 0 || want)) {
        const double tot = (S.red[0][tid] + S.red[1][tid]) + (S.red[2][tid] + S.red[3][tid]);
        if (tid == 0) {
            loss_vec[b] = live ? (float)(c * tot) : 0.f;
        } else {
            const int kind = (tid - 1) / MK, i = (tid - 1) % MK;
            if (i < K) {
                float gv = 0.f;
                if (live) gv = kind == 0 ? (float)(-c * S.kap[i] * tot) : kind == 1 ? (float)(-c * tot * S.pass[i]) : (float)(-c * tot);
                if (HEAD) {
                    (kind == 0 ? S.gmu : kind == 1 ? S.gkap : S.gw)[i] = gv;
                } else {
                    (kind == 0 ? d0 : kind == 1 ? d1 : d2)[o + i] = gv;
                }
            }
        }
    }

    // ---- (4) the head's backward: d0, d1, d2 = dpi_raw (B,K), dmu_raw (B,2K), dkappa_raw (B,K) ----
    if (HEAD && want) {
        __syncthreads();
        if (tid == 0)
            mvm_head_bwd_sample(in1 + 2 * o, in2 + o, S.hw, S.gmu, S.gkap, S.gw, K, temp, kappa_max, d0 + o, d1 + 2 * o, d2 + o);
    }
}

template <bool HEAD, typename... Args>
static void launch_grid_kl(int B, int maxK, hipStream_t st, Args... args) {
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, st, args...); };
    if (maxK == 1) launch(mvm_grid_kl_kernel<1, HEAD>);
    else if (maxK == 2) launch(mvm_grid_kl_kernel<2, HEAD>);
    else if (maxK <= 4) launch(mvm_grid_kl_kernel<4, HEAD>);
    else launch(mvm_grid_kl_kernel<8, HEAD>);
}

}  // namespace pnpp

using namespace pnpp;

extern "C" int pnpp_mvm_grid_kl(const float *mu, const float *kappa, const float *weight, const float *vm_gt, const int32_t *K_gt, int B,
                                int maxK, int num, float *loss_vec, float *dmu, float *dkappa, float *dweight, void *stream) {
    PNPP_REQUIRE(mu && kappa && weight && vm_gt && K_gt && loss_vec, PNPP_ERR_ARG, "mvm_grid_kl: null pointer");
    PNPP_REQUIRE((dmu && dkappa && dweight) || (!dmu && !dkappa && !dweight), PNPP_ERR_ARG,
                 "mvm_grid_kl: pass all three gradient outputs or none");
    PNPP_REQUIRE(B > 0, PNPP_ERR_ARG, "mvm_grid_kl: B=%d (1 <= B)", B);
    PNPP_REQUIRE(maxK >= 1 && maxK <= MATCH_KMAX, PNPP_ERR_ARG, "mvm_grid_kl: maxK=%d (1 <= maxK <= %d)", maxK, MATCH_KMAX);
    PNPP_REQUIRE(num >= 3 && num - 1 <= GKL_GMAX, PNPP_ERR_ARG, "mvm_grid_kl: num=%d (a grid of num - 1 points, 2 <= num - 1 <= %d)", num,
                 GKL_GMAX);
    ProfScope ps(as_stream(stream), "mvm_grid_kl_kernel B=%d K=%d G=%d", B, maxK, num - 1);
    launch_grid_kl<false>(B, maxK, as_stream(stream), mu, kappa, weight, vm_gt, K_gt, maxK, num - 1, 0.f, 0.f, loss_vec, dmu, dkappa,
                          dweight, (float *)nullptr, (float *)nullptr, (float *)nullptr);
    PNPP_CHECK_LAUNCH("mvm_grid_kl");
    return PNPP_OK;
}

extern "C" int pnpp_mvm_head_grid_kl(const float *pi_raw, const float *mu_raw, const float *kappa_raw, const float *vm_gt,
                                     const int32_t *K_gt, int B, int maxK, float temp, float kappa_max, int num, float *loss_vec,
                                     float *dpi_raw, float *dmu_raw, float *dkappa_raw, float *mu, float *kappa, float *weight,
                                     void *stream) {
    PNPP_REQUIRE(pi_raw && mu_raw && kappa_raw && vm_gt && K_gt && loss_vec, PNPP_ERR_ARG, "mvm_head_grid_kl: null pointer");
    PNPP_REQUIRE((dpi_raw && dmu_raw && dkappa_raw) || (!dpi_raw && !dmu_raw && !dkappa_raw), PNPP_ERR_ARG,
                 "mvm_head_grid_kl: pass all three gradient outputs or none");
    PNPP_REQUIRE((mu && kappa && weight) || (!mu && !kappa && !weight), PNPP_ERR_ARG,
                 "mvm_head_grid_kl: pass all three head outputs or none");
    PNPP_REQUIRE(B > 0, PNPP_ERR_ARG, "mvm_head_grid_kl: B=%d (1 <= B)", B);
    PNPP_REQUIRE(maxK >= 1 && maxK <= MATCH_KMAX, PNPP_ERR_ARG, "mvm_head_grid_kl: maxK=%d (1 <= maxK <= %d)", maxK, MATCH_KMAX);
    PNPP_REQUIRE(temp > 0.f, PNPP_ERR_ARG, "mvm_head_grid_kl: temp=%g (0 < temp)", (double)temp);
    PNPP_REQUIRE(num >= 3 && num - 1 <= GKL_GMAX, PNPP_ERR_ARG, "mvm_head_grid_kl: num=%d (a grid of num - 1 points, 2 <= num - 1 <= %d)",
                 num, GKL_GMAX);
    ProfScope ps(as_stream(stream), "mvm_head_grid_kl_kernel B=%d K=%d G=%d", B, maxK, num - 1);
    launch_grid_kl<true>(B, maxK, as_stream(stream), pi_raw, mu_raw, kappa_raw, vm_gt, K_gt, maxK, num - 1, temp, kappa_max, loss_vec,
                         dpi_raw, dmu_raw, dkappa_raw, mu, kappa, weight);
    PNPP_CHECK_LAUNCH("mvm_head_grid_kl");
    return PNPP_OK;
}
