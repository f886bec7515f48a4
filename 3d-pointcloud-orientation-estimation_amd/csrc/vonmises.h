// vonmises.h -- the float64 device math of the von-Mises heads and losses, shared by the stand-alone kernels (loss_kernels.hip) and the
// one-launch step tails (step_tail_kernels.hip): Bessel series, single- and multi-peak KL, the matching assignment, the multi-peak head
// of one sample.  Everything here is __forceinline__ or constexpr.
//
// All transcendental work is done in float64 (fp64 VALU is cheap on CDNA4 and B is tiny) and rounded once to float32.
//
// Bessel functions: exponentially scaled I0e / I1e by the Cephes Chebyshev expansions (the same
// tables ATen's torch.special.i0/i1 evaluate, BSD-licensed Cephes Math Library constants);
// log I0(k) = k + log(i0e(k)) never overflows, A(k) = I1/I0 = i1e/i0e, A'(k) = 1 - A^2 - A/k.
#pragma once
#include "common.h"

namespace pnpp {

constexpr double kI0eA[30] = {
    -4.41534164647933937950E-18, 3.33079451882223809783E-17,  -2.43127984654795469359E-16, 1.71539128555513303061E-15,
    -1.16853328779934516808E-14, 7.67618549860493561688E-14,  -4.85644678311192946090E-13, 2.95505266312963983461E-12,
    -1.72682629144155570723E-11, 9.67580903537323691224E-11,  -5.18979560163526290666E-10, 2.65982372468238665035E-9,
    -1.30002500998624804212E-8,  6.04699502254191894932E-8,   -2.67079385394061173391E-7,  1.11738753912010371815E-6,
    -4.41673835845875056359E-6,  1.64484480707288970893E-5,   -5.75419501008210370398E-5,  1.88502885095841655729E-4,
    -5.76375574538582365885E-4,  1.63947561694133579842E-3,   -4.32430999505057594430E-3,  1.05464603945949983183E-2,
    -2.37374148058994688156E-2,  4.93052842396707084878E-2,   -9.49010970480476444210E-2,  1.71620901522208775349E-1,
    -3.04682672343198398683E-1,  6.76795274409476084995E-1};
constexpr double kI0eB[25] = {
    -7.23318048787475395456E-18, -4.83050448594418207126E-18, 4.46562142029675999901E-17,  3.46122286769746109310E-17,
    -2.82762398051658348494E-16, -3.42548561967721913462E-16, 1.77256013305652638360E-15,  3.81168066935262242075E-15,
    -9.55484669882830764870E-15, -4.15056934728722208663E-14, 1.54008621752140982691E-14,  3.85277838274214270114E-13,
    7.18012445138366623367E-13,  -1.79417853150680611778E-12, -1.32158118404477131188E-11, -3.14991652796324136454E-11,
    1.18891471078464383424E-11,  4.94060238822496958910E-10,  3.39623202570838634515E-9,   2.26666899049817806459E-8,
    2.04891858946906374183E-7,   2.89137052083475648297E-6,   6.88975834691682398426E-5,   3.36911647825569408990E-3,
    8.04490411014108831608E-1};
constexpr double kI1eA[29] = {
    2.77791411276104639959E-18, -2.11142121435816608115E-17, 1.55363195773620046921E-16, -1.10559694773538630805E-15,
    7.60068429473540693410E-15, -5.04218550472791168711E-14, 3.22379336594557470981E-13, -1.98397439776494371520E-12,
    1.17361862988909016308E-11, -6.66348972350202774223E-11, 3.62559028155211703701E-10, -1.88724975172282928790E-9,
    9.38153738649577178388E-9,  -4.44505912879632808065E-8,  2.00329475355213526229E-7,  -8.56872026469545474066E-7,
    3.47025130813767847674E-6,  -1.32731636560394358279E-5,  4.78156510755005422638E-5,  -1.61760815825896745588E-4,
    5.12285956168575772895E-4,  -1.51357245063125314899E-3,  4.15642294431288815669E-3,  -1.05640848946261981558E-2,
    2.47264490306265168283E-2,  -5.29459812080949914269E-2,  1.02643658689847095384E-1,  -1.76416518357834055153E-1,
    2.52587186443633654823E-1};
constexpr double kI1eB[25] = {
    7.51729631084210481353E-18,  4.41434832307170791151E-18,  -4.65030536848935832153E-17, -3.20952592199342395980E-17,
    2.96262899764595013876E-16,  3.30820231092092828324E-16,  -1.88035477551078244854E-15, -3.81440307243700780478E-15,
    1.04202769841288027642E-14,  4.27244001671195135429E-14,  -2.10154184277266431302E-14, -4.08355111109219731823E-13,
    -7.19855177624590851209E-13, 2.03562854414708950722E-12,  1.41258074366137813316E-11,  3.25260358301548823856E-11,
    -1.89749581235054123450E-11, -5.58974346219658380687E-10, -3.83538038596423702205E-9,  -2.63146884688951950684E-8,
    -2.51223623787020892529E-7,  -3.88256480887769039346E-6,  -1.10588938762623716291E-4,  -9.76109749136146840777E-3,
    7.78576235018280120474E-1};

// Clenshaw recurrence, fully unrolled over a compile-time table: the coefficients become literals of the instruction stream.
// (Round 4: the tables used to be __device__ arrays read through a pointer inside a runtime loop -- one dependent scalar load per
// term, 25 - 30 terms, four series per KL value: a single kl_multi_eval took 20 - 35 us and the multi-peak loss was a 40 - 100 us
// launch.  Same operations in the same order; the values are unchanged.)
template <int N>
__device__ __forceinline__ double chbevl(double x, const double (&c)[N]) {
    double b0 = c[0], b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int i = 1; i < N; ++i) {
        b2 = b1;
        b1 = b0;
        b0 = x * b1 - b2 + c[i];
    }
    return 0.5 * (b0 - b2);
}
__device__ __forceinline__ double i0e(double x) {  // x >= 0
    return x <= 8.0 ? chbevl(0.5 * x - 2.0, kI0eA) : chbevl(32.0 / x - 2.0, kI0eB) / sqrt(x);
}
__device__ __forceinline__ double i1e(double x) {  // x >= 0
    return x <= 8.0 ? chbevl(0.5 * x - 2.0, kI1eA) * x : chbevl(32.0 / x - 2.0, kI1eB) / sqrt(x);
}
__device__ __forceinline__ double log_i0(double k) { return k + log(i0e(k)); }
__device__ __forceinline__ double bessel_ratio(double k) { return i1e(k) / i0e(k); }
__device__ __forceinline__ double bessel_ratio_prime(double k, double A) {
    return k > 1e-8 ? 1.0 - A * A - A / k : 0.5;
}

constexpr double kPi = 3.14159265358979323846;

// ---- single-peak KL, train_single_peak_vonMises_KL.py:23-28 --------------------------------------
__device__ __forceinline__ void kl_single_eval(double mp, double kp, double mq, double kq, double &kl, double &dmu,
                                               double &dk) {
    const double d = mp - mq;
    const double A = bessel_ratio(kp);
    const double base = log_i0(kq) - log_i0(kp);
    if (kp <= 1e-6) {  // a1 := 0 branch of line 26: only -log I0(kappa_p) depends on the prediction
        kl = base;
        dmu = 0.0;
        dk = -A;
    } else {
        const double cd = cos(d), sd = sin(d);
        kl = base + kp * A - kq * A * cd;
        dmu = kq * A * sd;
        dk = bessel_ratio_prime(kp, A) * (kp - kq * cd);
    }
}

// The float64 work of a sample is four independent chains of library calls and Chebyshev series (~5 us one after the other on one
// lane).  They cannot be spread over the lanes of a wave (different code per lane = divergence = serial again), so each of a
// 256-thread workgroup's four WAVES evaluates one chain for up to 64 samples, the pieces meet in LDS, and wave 0 combines them with
// the same float64 operations in the same order as kl_single_eval: bitwise the same result, a third of the latency.
struct KlPieces {
    double th[64], cd[64], sd[64], i0e_kp[64], logi0_kp[64], i1e_kp[64], logi0_kq[64], sig[64];
    float mu[64], kap[64];
};
// Called by ALL 256 threads (two barriers inside) for sample i = chunk base + lane; returns true on the wave-0 lane that owns a valid
// sample, with mu, kappa (float32, as the reference's head returns them), the loss value and d loss_mean / d o.
__device__ __forceinline__ bool vm_head_kl_chunk(KlPieces &S, int i, int B, double o0, double o1, const float *__restrict__ mu_gt,
                                                 const float *__restrict__ kappa_gt, double inv_b, float &mu_f, float &kap_f, float &vf,
                                                 float &g0, float &g1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (i < B) {
        if (wave == 0) {
            const double th = tanh(o0);
            const float m = (float)(th * kPi);                               // torch.tanh(out[:,0]) * np.pi
            const double d = (double)m - (double)mu_gt[i];
            S.th[lane] = th, S.cd[lane] = cos(d), S.sd[lane] = sin(d), S.mu[lane] = m;
        } else if (wave == 1) {
            const float k = (float)(o1 > 20.0 ? o1 : log1p(exp(o1)));        // F.softplus (beta 1, threshold 20)
            const double kp = (double)k, e0 = i0e(kp);
            S.i0e_kp[lane] = e0, S.logi0_kp[lane] = kp + log(e0), S.kap[lane] = k;
        } else if (wave == 2) {
            const float k = (float)(o1 > 20.0 ? o1 : log1p(exp(o1)));
            S.i1e_kp[lane] = i1e((double)k);
        } else {
            S.logi0_kq[lane] = log_i0((double)kappa_gt[i]);
            S.sig[lane] = o1 > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-o1));
        }
    }
    __syncthreads();
    bool mine = false;
    if (wave == 0 && i < B) {
        mine = true;
        const double th = S.th[lane], cd = S.cd[lane], sd = S.sd[lane];
        mu_f = S.mu[lane], kap_f = S.kap[lane];
        const double kp = (double)kap_f, kq = (double)kappa_gt[i];
        const double A = S.i1e_kp[lane] / S.i0e_kp[lane];          // bessel_ratio(kp)
        const double basev = S.logi0_kq[lane] - S.logi0_kp[lane];  // log I0(kq) - log I0(kp)
        double v, a, b;
        if (kp <= 1e-6) {
            v = basev, a = 0.0, b = -A;
        } else {
            v = basev + kp * A - kq * A * cd;
            a = kq * A * sd;
            b = bessel_ratio_prime(kp, A) * (kp - kq * cd);
        }
        vf = (float)v;
        g0 = (float)(a * kPi * (1.0 - th * th) * inv_b);
        g1 = (float)(b * S.sig[lane] * inv_b);
    }
    __syncthreads();
    return mine;
}

// ---- multi-peak KL + matching, train_multi_peaks_vonMises_KL.py:38-81 ----------------------------
constexpr int MATCH_KMAX = 8;

__device__ __forceinline__ void kl_multi_eval(double mp, double kp_raw, double mq, double kq_raw, double &kl, double &dmu,
                                              double &dk) {
    // torch.clamp keeps a NaN (fmax / fmin would return the other operand and turn it into 1e-6): it has to reach nan_to_num
    auto clamp_k = [](double k) -> double { return k < 1e-6 ? 1e-6 : k > 500.0 ? 500.0 : k; };
    const double kp = clamp_k(kp_raw), kq = clamp_k(kq_raw);
    double d = fmod(mp - mq + kPi, 2.0 * kPi);  // python %: result takes the sign of the divisor
    if (d < 0.0) d += 2.0 * kPi;
    d -= kPi;
    const double A = bessel_ratio(kp);
    const double cd = cos(d), sd = sin(d);
    kl = (log_i0(kq) - log_i0(kp)) + A * (kp - kq * cd);
    dmu = A * kq * sd;
    const bool pass = kp_raw >= 1e-6 && kp_raw <= 500.0;  // clamp backward
    dk = pass ? bessel_ratio_prime(kp, A) * (kp - kq * cd) : 0.0;
}

// match_loss of one sample in two parts, because the first is what costs: the K x K cost matrix is K^2 independent evaluations of
// kl_multi_eval (two Bessel series, log, cos / sin in float64: ~4 us each on one lane) -- sixteen in a row per sample made the
// one-thread-per-sample kernel a 60 - 100 us launch with 32 lanes of the chip busy (round 4: the largest launch of configs[2]'s step).
// So (1) one THREAD PER MATRIX ENTRY fills cost / gradient tables in LDS, (2) one thread per sample does the assignment and the
// weighted reduction from the tables.  Entry by entry the arithmetic is what the serial form did.
__device__ __forceinline__ void match_cost_entry(float mu_i, float kappa_i, float mq, float kq, float &cost, float &gmu, float &gk) {
    double v, a, c;
    kl_multi_eval((double)mu_i, (double)kappa_i, (double)mq, (double)kq, v, a, c);
    float vf = (float)v;   // rounded to float32 like the reference's cost tensor (line 66-73)
    if (!(fabsf(vf) <= 3.0e38f)) {  // nan_to_num(nan/+-inf -> 1e6): constant, no gradient
        vf = 1e6f;
        a = 0.0;
        c = 0.0;
    }
    cost = vf, gmu = (float)a, gk = (float)c;
}

// cost / gmu / gk: this sample's tables, entry (i, j) at [i * maxK + j], filled for i, j < K.  w (maxK); outputs may be null.
// MK: compile-time bound of maxK.  Everything per-sample lives in REGISTERS: the permutation is eight 4-bit fields of one word and
// every loop over components runs to MK under an `i < K` test, so no array is indexed by a run-time value (round 4: `int perm[8]`
// and friends lived in scratch memory -- a global-memory round trip per access, 24 permutations x ~20 accesses: 42 us of the
// multi-peak step's 71 us tail launch by in-kernel stamps, tools/tail_stamps.py).
template <int MK>
__device__ __forceinline__ void match_assign_sample(const float *cost, const float *gmu, const float *gk, const float *w, int K, int maxK,
                                                    float *loss, float *dmu, float *dkappa, float *dw, int32_t *assign) {
    if (K > maxK) K = maxK;
#pragma unroll
    for (int i = 0; i < MK; ++i)
        if (i < maxK) {
            if (dmu) dmu[i] = 0.f;
            if (dkappa) dkappa[i] = 0.f;
            if (dw) dw[i] = 0.f;
            if (assign) assign[i] = -1;
        }
    if (K <= 0) {
        *loss = 0.f;
        return;
    }
    auto nib = [](unsigned p, int i) -> int { return (int)((p >> (4 * i)) & 15u); };
    auto swp = [](unsigned p, int i, int j) -> unsigned {
        const unsigned x = ((p >> (4 * i)) ^ (p >> (4 * j))) & 15u;
        return p ^ ((x << (4 * i)) | (x << (4 * j)));
    };
    // exhaustive optimal assignment in lexicographic permutation order, first optimum kept
    unsigned perm = 0x76543210u, bestp = perm;
    double best = 1e300;
    while (true) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < MK; ++i)
            if (i < K) t += (double)cost[i * maxK + nib(perm, i)];
        if (t < best) best = t, bestp = perm;
        int i = K - 2;  // next lexicographic permutation of the first K fields
        while (i >= 0 && nib(perm, i) > nib(perm, i + 1)) --i;
        if (i < 0) break;
        int j = K - 1;
        while (nib(perm, j) < nib(perm, i)) --j;
        perm = swp(perm, i, j);
        for (int l = i + 1, r = K - 1; l < r; ++l, --r) perm = swp(perm, l, r);
    }
    // loss_b = sum w_i c_i / (sum w_i + 1e-8)   (float32 arithmetic order of lines 77-80, evaluated in double)
    double sw = 0.0, swc = 0.0;
#pragma unroll
    for (int i = 0; i < MK; ++i)
        if (i < K) {
            sw += (double)w[i];
            swc += (double)w[i] * (double)cost[i * maxK + nib(bestp, i)];
        }
    const double S = sw + 1e-8;
    *loss = (float)(swc / S);
#pragma unroll
    for (int i = 0; i < MK; ++i)
        if (i < K) {
            const double wi = (double)w[i];
            const int j = nib(bestp, i);
            if (assign) assign[i] = j;
            if (dw) dw[i] = (float)(((double)cost[i * maxK + j] * S - swc) / (S * S));
            if (dmu) dmu[i] = (float)(wi / S * (double)gmu[i * maxK + j]);
            if (dkappa) dkappa[i] = (float)(wi / S * (double)gk[i * maxK + j]);
        }
}

// ---- multi-peak output head, pointnet_pp_mvM.py:91-125 ---------------------------------------------
// one sample: pi_raw (K), mu_raw (K x 2), kappa_raw (K) -> mu, kappa, weight (K)
__device__ __forceinline__ void mvm_head_sample(const float *pi_raw, const float *mu_raw, const float *kappa_raw, int K, float temp,
                                                float kappa_max, float *mu, float *kappa, float *weight) {
    double mx = -1e300;
    for (int k = 0; k < K; ++k) mx = fmax(mx, (double)pi_raw[k] / (double)temp);
    double se = 0.0;
    for (int k = 0; k < K; ++k) se += exp((double)pi_raw[k] / (double)temp - mx);
    for (int k = 0; k < K; ++k) {
        weight[k] = (float)(exp((double)pi_raw[k] / (double)temp - mx) / se);
        const float c0 = mu_raw[k * 2], s0 = mu_raw[k * 2 + 1];
        const float nrm = fmaxf(sqrtf(c0 * c0 + s0 * s0), 1e-4f);  // F.normalize(eps=1e-4)
        float c = c0 / nrm, s = s0 / nrm;
        if (sqrtf(c * c + s * s) < 1e-3f) c = 1.f, s = 0.f;        // degenerate direction -> mu = 0
        mu[k] = (float)atan2((double)s, (double)c);
        const double kr = (double)kappa_raw[k];
        const double sp = (kr > 20.0 ? kr : log1p(exp(kr))) + 1e-6;
        kappa[k] = (float)fmin(sp, (double)kappa_max);
    }
}

// one sample: gradients w.r.t. the raw head outputs from (dmu, dkappa, dweight)
__device__ __forceinline__ void mvm_head_bwd_sample(const float *mu_raw, const float *kappa_raw, const float *weight, const float *dmu,
                                                    const float *dkappa, const float *dweight, int K, float temp, float kappa_max,
                                                    float *dpi_raw, float *dmu_raw, float *dkappa_raw) {
    double dot = 0.0;
    for (int k = 0; k < K; ++k) dot += (double)weight[k] * (double)dweight[k];
    for (int k = 0; k < K; ++k) {
        const double wk = (double)weight[k];
        dpi_raw[k] = (float)(wk * ((double)dweight[k] - dot) / (double)temp);
        // atan2(s, c) with (c, s) = r / max(|r|, eps)
        const double r0 = (double)mu_raw[k * 2], r1 = (double)mu_raw[k * 2 + 1];
        const double n = sqrt(r0 * r0 + r1 * r1);
        const double den = fmax(n, 1e-4);
        const double c = r0 / den, s = r1 / den;
        const double n2 = c * c + s * s;
        double g0 = 0.0, g1 = 0.0;
        if (sqrt(n2) >= 1e-3) {
            const double gm = (double)dmu[k];
            const double dc = -s / n2 * gm, ds = c / n2 * gm;  // d atan2 / d(c, s)
            if (n >= 1e-4) {                                   // u = r/|r|: (I - u u^T)/|r|
                const double proj = dc * c + ds * s;
                g0 = (dc - c * proj) / n;
                g1 = (ds - s * proj) / n;
            } else {                                           // u = r/eps
                g0 = dc / 1e-4;
                g1 = ds / 1e-4;
            }
        }
        dmu_raw[k * 2] = (float)g0;
        dmu_raw[k * 2 + 1] = (float)g1;
        const double kr = (double)kappa_raw[k];
        const double sp = (kr > 20.0 ? kr : log1p(exp(kr))) + 1e-6;
        const double sig = kr > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-kr));
        dkappa_raw[k] = (float)(sp <= (double)kappa_max ? (double)dkappa[k] * sig : 0.0);
    }
}

}  // namespace pnpp
