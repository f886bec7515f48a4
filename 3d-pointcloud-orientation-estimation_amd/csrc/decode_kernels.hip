// decode_kernels.hip -- from von-Mises parameters to orientations, and from orientations to angular errors.
//
// mvm_decode_kernel: the modes of a mixture density p(theta) = sum_k w_k vM(theta; mu_k, kappa_k) of one sample: the density on
// the reference's grid (models/pointnet_pp_mvM.py:131-144, with exp(kappa cos) / I0(kappa) written as exp(kappa (cos - 1)) / i0e(kappa)
// so that nothing overflows), its circular local maxima refined by value sectioning, sorted, cut and wrapped.
// orient_eval_kernel: per-sample angular errors against the ground truth and their histograms / counts in a device-resident
// accumulator of 64-bit integers (order-independent, so a summary is bit-reproducible).
//
// All arithmetic on angles and densities is float64, rounded once to float32 on the way out (vonmises.h says why that is cheap here).
#include "kernels.h"
#include "vonmises.h"

namespace pnpp {

constexpr int DEC_GMAX = 1024;     // grid points of a sample (num - 1)
constexpr int DEC_CMAX = DEC_GMAX / 2;   // a circular sequence of G values has at most G / 2 strict-rise local maxima
constexpr int DEC_ROUNDS = 8;      // value-sectioning rounds: the bracket shrinks 32 x per round
constexpr double kTwoPi = 2.0 * kPi;

struct DecodeShared {
    double p[DEC_GMAX];            // unnormalised density on the grid
    double ang[DEC_CMAX], hgt[DEC_CMAX];   // refined candidates
    double mu[MATCH_KMAX], kap[MATCH_KMAX], coef[MATCH_KMAX];   // coef = w / (2 pi i0e(kappa)); 0 beyond the components in use
    double red[4];
    unsigned long long mask[DEC_GMAX / 64];   // candidate ballots, one word per 64 consecutive grid points
    int cand[DEC_CMAX];            // grid index of each candidate, in grid order
};

// p(x), unnormalised.  KT: the compile-time bound of K (1, 2, 4 or 8).  The loop is fully unrolled with NO test inside: a component
// that is not in use has coef = kappa = mu = 0 and adds an exact +0, and without branches between them the KT chains of float64
// cos / exp interleave in the instruction stream -- the evaluation is latency-bound, one wave per SIMD.  The tables are read at
// compile-time offsets (LDS broadcasts): nothing is indexed by a run-time value.
template <int KT>
__device__ __forceinline__ double mix_eval(const DecodeShared &S, double x) {
    double p = 0.0;
#pragma unroll
    for (int k = 0; k < KT; ++k) p += S.coef[k] * exp(S.kap[k] * (cos(x - S.mu[k]) - 1.0));
    return p;
}

// One workgroup of four waves per sample.  (1) the component tables, (2) the grid into LDS + the row sum, (3) candidates compacted in
// grid order by ballots, (4) each wave refines one candidate at a time: a round is one 64-lane evaluation and a wave arg-max,
// (5) wave 0 picks the K highest in order.
template <int KT>
__global__ void __launch_bounds__(256) mvm_decode_kernel(const float *__restrict__ mu, const float *__restrict__ kappa,
                                                         const float *__restrict__ weight, const int32_t *__restrict__ counts, int K,
                                                         int G, float rel_height, float *__restrict__ modes,
                                                         float *__restrict__ heights, int32_t *__restrict__ n_modes,
                                                         float *__restrict__ angle, float *__restrict__ density) {
    __shared__ DecodeShared S;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cnt = counts ? counts[b] : K;
    cnt = cnt < 0 ? 0 : cnt > K ? K : cnt;
    if (tid < MATCH_KMAX) {
        double m = 0.0, kp = 0.0, c = 0.0;
        if (tid < cnt) {
            m = (double)mu[(size_t)b * K + tid];
            const double kr = (double)kappa[(size_t)b * K + tid];
            kp = kr > 0.0 ? kr : 0.0;   // a negative or NaN concentration counts as 0 (i0e takes x >= 0)
            const double w = weight ? (double)weight[(size_t)b * K + tid] : 1.0;
            c = w / (kTwoPi * i0e(kp));
        }
        S.mu[tid] = m, S.kap[tid] = kp, S.coef[tid] = c;
    }
    __syncthreads();

    // ---- (2) the grid ----
    const double step = kTwoPi / (double)G;
    double part = 0.0;
    for (int i = tid; i < G; i += 256) {
        const double v = mix_eval<KT>(S, (double)i * kTwoPi / (double)G);
        S.p[i] = v;
        part += v;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += shfl_xor_f64(part, m);
    if (lane == 0) S.red[wave] = part;
    __syncthreads();
    if (density) {
        const double tot = ((S.red[0] + S.red[1]) + (S.red[2] + S.red[3])) + 1e-8;
        for (int i = tid; i < G; i += 256) density[(size_t)b * G + i] = (float)(S.p[i] / tot);
    }

    // ---- (3) candidates: p_i > p_{i-1} and p_i >= p_{i+1}, circular ----
    const int nchunk = (G + 63) >> 6;   // <= 16
    for (int ch = wave; ch < nchunk; ch += 4) {
        const int i = ch * 64 + lane;
        bool c = false;
        if (i < G) {
            const double v = S.p[i], l = S.p[i == 0 ? G - 1 : i - 1], r = S.p[i == G - 1 ? 0 : i + 1];
            c = v > l && v >= r;
        }
        const unsigned long long m = __ballot(c);
        if (lane == 0) S.mask[ch] = m;
    }
    __syncthreads();
    int ncand = 0;
    for (int ch = 0; ch < nchunk; ++ch) {
        const unsigned long long m = S.mask[ch];
        if ((ch & 3) == wave && ((m >> lane) & 1ull))
            S.cand[ncand + __popcll(m & ((1ull << lane) - 1ull))] = ch * 64 + lane;
        ncand += __popcll(m);
    }
    __syncthreads();

    // ---- (4) value sectioning inside [theta_{i-1}, theta_{i+1}] ----
    // 65 equispaced points per round: lanes 1..63 evaluate the interior ones; the two end points are points of the round before (of
    // the grid, in round 1) and their values are carried, not evaluated again.
    for (int c = wave; c < ncand; c += 4) {
        const int i = S.cand[c];
        const double th = (double)i * kTwoPi / (double)G;
        double a = th - step, w = 2.0 * step;
        double v0 = S.p[i == 0 ? G - 1 : i - 1], v64 = S.p[i == G - 1 ? 0 : i + 1];
        for (int r = 0; r < DEC_ROUNDS; ++r) {
            const double d = w * (1.0 / 64.0);
            double v = lane == 0 ? v0 : mix_eval<KT>(S, a + (double)lane * d);
            // wave arg-max, the first on ties
            double bv = v;
            int bj = lane;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double ov = shfl_xor_f64(bv, m);
                const int oj = __shfl_xor(bj, m, 64);
                if (ov > bv || (ov == bv && oj < bj)) bv = ov, bj = oj;
            }
            if (v64 > bv) bj = 64;
            bj = bj < 1 ? 1 : bj > 63 ? 63 : bj;
            const double lo_v = __hiloint2double(__shfl(__double2hiint(v), bj - 1, 64), __shfl(__double2loint(v), bj - 1, 64));
            const double hi_v = __hiloint2double(__shfl(__double2hiint(v), (bj + 1) & 63, 64), __shfl(__double2loint(v), (bj + 1) & 63, 64));
            v0 = lo_v;
            if (bj + 1 < 64) v64 = hi_v;
            a += (double)(bj - 1) * d;
            w = 2.0 * d;
        }
        const double mid = a + 0.5 * w;
        const double h = mix_eval<KT>(S, mid);
        if (lane == 0) {
            double x = mid;   // into [0, 2 pi): the order of equal heights
            if (x < 0.0) x += kTwoPi;
            if (x >= kTwoPi) x -= kTwoPi;
            S.ang[c] = x, S.hgt[c] = h;
        }
    }
    __syncthreads();

    // ---- (5) the K highest by (height descending, angle ascending); cut at rel_height x the top; wrap to (-pi, pi] ----
    if (wave == 0) {
        double top = 0.0;
        int n = 0;
        bool open = true;
        for (int s = 0; s < K; ++s) {
            double bh = -1.0, ba = 0.0;
            int bc = -1;
            if (open)
                for (int c = lane; c < ncand; c += 64) {
                    const double h = S.hgt[c], x = S.ang[c];
                    if (h > bh || (h == bh && x < ba)) bh = h, ba = x, bc = c;
                }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double oh = shfl_xor_f64(bh, m), oa = shfl_xor_f64(ba, m);
                const int oc = __shfl_xor(bc, m, 64);
                if (oh > bh || (oh == bh && oc >= 0 && (bc < 0 || oa < ba))) bh = oh, ba = oa, bc = oc;
            }
            if (s == 0) top = bh;
            const bool keep = open && bc >= 0 && bh >= (double)rel_height * top;
            if (!keep) open = false;
            if (keep) {
                ++n;
                if (lane == 0) S.hgt[bc] = -2.0;   // taken
            }
            if (lane == 0) {
                const double x = ba > kPi ? ba - kTwoPi : ba;
                modes[(size_t)b * K + s] = keep ? (float)x : __builtin_nanf("");
                heights[(size_t)b * K + s] = keep ? (float)bh : 0.f;
                if (s == 0 && angle) angle[b] = keep ? (float)x : __builtin_nanf("");
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0) n_modes[b] = n;
    }
}

// ---- angular errors -------------------------------------------------------------------------------------------------------
// The accumulator: int64 words, label l's block at acc + l * ORI_STRIDE = [top1 histogram (360) | cover histogram (360) | included,
// excluded, count_ok, sum of top1 in micro-degrees, sum of cover in micro-degrees | 3 spare]; after the n_labels blocks one word, the
// cursor of the per-sample buffer.
constexpr int ORI_BINS = PNPP_ORIENT_BINS, ORI_STRIDE = PNPP_ORIENT_STRIDE;

__device__ __forceinline__ double wrap_abs(double d) {   // |wrap(d)| in [0, pi]
    d -= kTwoPi * rint(d / kTwoPi);
    return fabs(d);
}

// ONE workgroup: the cursor is read before and advanced after, so sample i of a launch always lands at cursor + i.
__global__ void __launch_bounds__(256) orient_eval_kernel(const float *__restrict__ modes, const int32_t *__restrict__ n_modes,
                                                          const float *__restrict__ angle, int K, const float *__restrict__ mu_gt,
                                                          const float *__restrict__ kappa_gt, const float *__restrict__ vm_gt,
                                                          const int32_t *__restrict__ K_gt, int Kmax,
                                                          const int32_t *__restrict__ labels, int B, int n_labels,
                                                          unsigned long long *__restrict__ acc, float *__restrict__ sample_err,
                                                          long long capacity, float *__restrict__ top1_out,
                                                          float *__restrict__ cover_out, int32_t *__restrict__ count_ok_out) {
    unsigned long long *cursor = acc ? acc + (size_t)n_labels * ORI_STRIDE : nullptr;
    const unsigned long long base = cursor ? *cursor : 0ull;
    __syncthreads();   // everyone has the cursor before thread 0 moves it
    for (int i = threadIdx.x; i < B; i += 256) {
        const int nm = min(max(n_modes[i], 0), K);
        int kg = vm_gt ? min(max(K_gt[i], 0), Kmax) : 1;
        const int kg_raw = vm_gt ? K_gt[i] : 1;
        bool any = false;
        double top1 = 1e300, cover = 0.0;
        const double a0 = (double)angle[i];
        for (int j = 0; j < kg; ++j) {
            const double m = vm_gt ? (double)vm_gt[((size_t)i * Kmax + j) * 3] : (double)mu_gt[i];
            const double kq = vm_gt ? (double)vm_gt[((size_t)i * Kmax + j) * 3 + 1] : (double)kappa_gt[i];
            any = any || kq > 1e-6;
            top1 = fmin(top1, wrap_abs(a0 - m));
            double near = 1e300;
            for (int s = 0; s < nm; ++s) near = fmin(near, wrap_abs((double)modes[(size_t)i * K + s] - m));
            cover = fmax(cover, near);
        }
        const bool incl = kg > 0 && any && nm > 0 && top1 <= 4.0 && cover <= 4.0;   // a NaN in the ground truth fails the comparisons
        const double t_deg = incl ? top1 * (180.0 / kPi) : -1.0, c_deg = incl ? cover * (180.0 / kPi) : -1.0;
        const int ok = nm == kg_raw ? 1 : 0;
        if (top1_out) top1_out[i] = (float)t_deg;
        if (cover_out) cover_out[i] = (float)c_deg;
        if (count_ok_out) count_ok_out[i] = ok;
        if (!acc) continue;
        int l = labels ? labels[i] : 0;
        l = l < 0 ? 0 : l >= n_labels ? n_labels - 1 : l;   // a label outside the table cannot write outside it
        unsigned long long *A = acc + (size_t)l * ORI_STRIDE;
        if (incl) {
            const int bt = min(max((int)(t_deg * 2.0), 0), ORI_BINS - 1), bc = min(max((int)(c_deg * 2.0), 0), ORI_BINS - 1);
            atomicAdd(A + bt, 1ull);
            atomicAdd(A + ORI_BINS + bc, 1ull);
            atomicAdd(A + 2 * ORI_BINS, 1ull);
            atomicAdd(A + 2 * ORI_BINS + 3, (unsigned long long)llrint(t_deg * 1e6));
            atomicAdd(A + 2 * ORI_BINS + 4, (unsigned long long)llrint(c_deg * 1e6));
        } else {
            atomicAdd(A + 2 * ORI_BINS + 1, 1ull);
        }
        if (ok) atomicAdd(A + 2 * ORI_BINS + 2, 1ull);
        if (sample_err && base + (unsigned long long)i < (unsigned long long)capacity) {
            sample_err[2 * (base + i)] = (float)t_deg;
            sample_err[2 * (base + i) + 1] = (float)c_deg;
        }
    }
    if (cursor && threadIdx.x == 0) *cursor = base + (unsigned long long)B;
}

}  // namespace pnpp

using namespace pnpp;

extern "C" int pnpp_mvm_decode(const float *mu, const float *kappa, const float *weight, const int32_t *counts, int B, int K, int num,
                               float rel_height, float *modes, float *heights, int32_t *n_modes, float *angle, float *density,
                               void *stream) {
    PNPP_REQUIRE(mu && kappa && modes && heights && n_modes, PNPP_ERR_ARG, "mvm_decode: null pointer");
    PNPP_REQUIRE(B > 0, PNPP_ERR_ARG, "mvm_decode: B=%d (1 <= B)", B);
    PNPP_REQUIRE(K >= 1 && K <= MATCH_KMAX, PNPP_ERR_ARG, "mvm_decode: K=%d (1 <= K <= %d)", K, MATCH_KMAX);
    PNPP_REQUIRE(weight || K == 1, PNPP_ERR_ARG, "mvm_decode: null weight takes K=1, got K=%d", K);
    PNPP_REQUIRE(num >= 3 && num - 1 <= DEC_GMAX, PNPP_ERR_ARG, "mvm_decode: num=%d (a grid of num - 1 points, 2 <= num - 1 <= %d)", num,
                 DEC_GMAX);
    PNPP_REQUIRE(rel_height >= 0.f && rel_height <= 1.f, PNPP_ERR_ARG, "mvm_decode: rel_height=%g (0 <= rel_height <= 1)",
                 (double)rel_height);
    ProfScope ps(as_stream(stream), "mvm_decode_kernel B=%d K=%d G=%d", B, K, num - 1);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, as_stream(stream), mu, kappa, weight, counts, K, num - 1, rel_height, modes,
                           heights, n_modes, angle, density);
    };
    if (K == 1) launch(mvm_decode_kernel<1>);
    else if (K == 2) launch(mvm_decode_kernel<2>);
    else if (K <= 4) launch(mvm_decode_kernel<4>);
    else launch(mvm_decode_kernel<8>);
    PNPP_CHECK_LAUNCH("mvm_decode");
    return PNPP_OK;
}

extern "C" int pnpp_orient_eval(const float *modes, const int32_t *n_modes, const float *angle, int B, int K, const float *mu_gt,
                                const float *kappa_gt, const float *vm_gt, const int32_t *K_gt, int Kmax, const int32_t *labels,
                                int n_labels, uint64_t *acc, float *sample_err, int64_t capacity, float *top1, float *cover,
                                int32_t *count_ok, void *stream) {
    PNPP_REQUIRE(modes && n_modes && angle, PNPP_ERR_ARG, "orient_eval: null pointer");
    PNPP_REQUIRE(B > 0, PNPP_ERR_ARG, "orient_eval: B=%d (1 <= B)", B);
    PNPP_REQUIRE(K >= 1 && K <= MATCH_KMAX, PNPP_ERR_ARG, "orient_eval: K=%d (1 <= K <= %d)", K, MATCH_KMAX);
    const bool single = mu_gt || kappa_gt, multi = vm_gt || K_gt;
    PNPP_REQUIRE(single != multi, PNPP_ERR_ARG, "orient_eval: pass either mu_gt and kappa_gt or vm_gt and K_gt");
    PNPP_REQUIRE(!single || (mu_gt && kappa_gt), PNPP_ERR_ARG, "orient_eval: mu_gt and kappa_gt go together");
    PNPP_REQUIRE(!multi || (vm_gt && K_gt), PNPP_ERR_ARG, "orient_eval: vm_gt and K_gt go together");
    PNPP_REQUIRE(!multi || (Kmax >= 1 && Kmax <= MATCH_KMAX), PNPP_ERR_ARG, "orient_eval: Kmax=%d (1 <= Kmax <= %d)", Kmax, MATCH_KMAX);
    PNPP_REQUIRE(acc || top1 || cover || count_ok, PNPP_ERR_ARG, "orient_eval: no output requested");
    PNPP_REQUIRE(!acc || (n_labels >= 1 && n_labels <= PNPP_ORIENT_MAX_LABELS), PNPP_ERR_ARG, "orient_eval: n_labels=%d (1 <= n_labels <= %d)",
                 n_labels, PNPP_ORIENT_MAX_LABELS);
    PNPP_REQUIRE(acc || !sample_err, PNPP_ERR_ARG, "orient_eval: the per-sample buffer needs the accumulator (its cursor)");
    PNPP_REQUIRE(!sample_err || capacity > 0, PNPP_ERR_ARG, "orient_eval: capacity=%lld of the per-sample buffer", (long long)capacity);
    ProfScope ps(as_stream(stream), "orient_eval_kernel B=%d K=%d", B, K);
    hipLaunchKernelGGL(orient_eval_kernel, dim3(1), dim3(256), 0, as_stream(stream), modes, n_modes, angle, K, mu_gt, kappa_gt, vm_gt, K_gt,
                       Kmax, labels, B, n_labels, reinterpret_cast<unsigned long long *>(acc), sample_err, (long long)capacity, top1,
                       cover, count_ok);
    PNPP_CHECK_LAUNCH("orient_eval");
    return PNPP_OK;
}
