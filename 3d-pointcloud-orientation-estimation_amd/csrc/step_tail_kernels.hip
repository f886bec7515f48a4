// step_tail_kernels.hip -- the two one-launch tails that close a training step: output head(s), loss, batch mean and their backward in
// a single workgroup, with the NEXT step's centre draw (sampler_device.h) riding in the launch's other workgroups.  The per-sample
// arithmetic is that of the stand-alone kernels of loss_kernels.hip: the same device functions (vonmises.h).  One stand-alone kernel
// lives here too: vm_match_loss_kernel (see the note at it).
#include <optional>

#include "kernels.h"
#include "sampler_device.h"
#include "vonmises.h"

namespace pnpp {

#ifdef PNPP_STAMPS
__device__ unsigned long long g_tail_stamps[16];   // s_memtime ticks of thread 0 of the tail workgroup, per phase
#define TAIL_STAMP(i)                                                        \
    if (threadIdx.x == 0) {                                                  \
        const unsigned long long st_t = __builtin_amdgcn_s_memtime();        \
        g_tail_stamps[i] += st_t - st_last;                                  \
        st_last = st_t;                                                      \
    }
#else
#define TAIL_STAMP(i)
#endif

// The whole tail of the single-peak training step in ONE single-workgroup launch: o = x W^T + b (the model's fc3,
// pointnet_pp_vonMises.py:35), head activations, KL, batch mean (train_single_peak_vonMises_KL.py:82-84) and their
// backward -- d loss / d W, d b and d x.  x: (B, K) features, W: (2, K).  Eager PyTorch terms: a Linear, the head,
// the loss, a mean and seven autograd nodes.  The mean is a fixed-order fp64 tree; everything is deterministic.
__global__ void __launch_bounds__(256)
vm_fc_head_kl_step_kernel(const float *__restrict__ x, const float *__restrict__ W, const float *__restrict__ bias,
                          const float *__restrict__ mu_gt, const float *__restrict__ kappa_gt, int B, int K, int x_in_lds,
                          float *__restrict__ loss_mean, float *__restrict__ dW, float *__restrict__ db, float *__restrict__ dx,
                          const SampleJob J) {
    extern __shared__ __attribute__((aligned(16))) float sm[];  // o[B][2] (then d_o in place), xs[B][K] when it fits
    // The tail is ONE workgroup on a 256-CU chip.  The centre draw of the NEXT step (models/pointnet_pp_8dir.py:28 of sa1 and sa2)
    // depends on nothing but its counter, so its 2 B workgroups ride in this launch (blocks 1 ..) instead of opening the next step
    // with a launch of their own: same draws, same order, one launch and ~7 us fewer per step.
    if (blockIdx.x > 0) {
        __shared__ int nc_s;
        sample_random_body(J.seed_lo, J.seed_hi, J.str_lo, J.str_hi, J.str_dev, J.N1, J.npoint1, J.out1, J.B, J.N2, J.npoint2, J.out2,
                           (int)blockIdx.x - 1, (int)gridDim.x - 1, reinterpret_cast<unsigned long long *>(sm), nc_s);
        return;
    }
    __shared__ double red[256];
    float *o = sm;
    float *ws = sm + ((2 * B + 3) & ~3);         // W (2 x K) in LDS: with x, ONE round trip for everything the kernel reads
    float *xs = ws + ((2 * K + 3) & ~3);
    const int tid = threadIdx.x;
#ifdef PNPP_STAMPS
    unsigned long long st_last = __builtin_amdgcn_s_memtime();
#endif
    const float *xr = x;  // where the features are read from after staging
    for (int f = tid; f < 2 * K; f += 256) ws[f] = W[f];
    const float b0 = bias[0], b1 = bias[1];
    if (x_in_lds) {       // one pass of independent 16-byte loads; every later read of x is an LDS read
        const int n4 = (B * K) >> 2;
        for (int f = tid; f < n4; f += 256) reinterpret_cast<float4 *>(xs)[f] = reinterpret_cast<const float4 *>(x)[f];
        xr = xs;
    }
    __syncthreads();
    TAIL_STAMP(8)   // staging
    const float *Wl = ws;
    // 1. o = x W^T + b: eight lanes per row, each a strided eighth of the features
    const int part8 = tid & 7;
    for (int i = tid >> 3; i < ((B + 31) & ~31); i += 32) {
        const int ic = min(i, B - 1);
        float a0 = 0.f, a1 = 0.f;
        for (int k = part8; k < K; k += 8) {
            const float xv = xr[(size_t)ic * K + k];
            a0 = fmaf(xv, Wl[k], a0), a1 = fmaf(xv, Wl[K + k], a1);
        }
#pragma unroll
        for (int m = 4; m >= 1; m >>= 1) a0 += __shfl_xor(a0, m), a1 += __shfl_xor(a1, m);
        if (part8 == 0 && i < B) o[2 * i] = a0 + b0, o[2 * i + 1] = a1 + b1;
    }
    __syncthreads();
    TAIL_STAMP(9)   // o = x W^T
    // 2. head + KL + mean (the four float64 chains on the four waves: vm_head_kl_chunk); d loss / d o overwrites o
    __shared__ KlPieces S;
    const double inv_b = 1.0 / (double)B;
    double part = 0.0;
    for (int base = 0; base < B; base += 64) {
        const int i = base + (tid & 63);
        const double o0 = i < B ? (double)o[2 * i] : 0.0, o1 = i < B ? (double)o[2 * i + 1] : 0.0;
        float mu_f, kap_f, vf, g0, g1;
        if (vm_head_kl_chunk(S, i, B, o0, o1, mu_gt, kappa_gt, inv_b, mu_f, kap_f, vf, g0, g1)) {
            part += (double)vf;
            o[2 * i] = g0;      // (every wave read o[2i], o[2i+1] before the first barrier of the chunk)
            o[2 * i + 1] = g1;
        }
    }
    TAIL_STAMP(10)   // head + KL
    red[tid] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) *loss_mean = (float)(red[0] * inv_b);
    TAIL_STAMP(11)   // mean
    // 3. dW = d_o^T x, db = column sums of d_o, dx = d_o W: one thread per feature, rows in order
    for (int k = tid; k < K; k += 256) {
        const float w0 = Wl[k], w1 = Wl[K + k];
        float g0 = 0.f, g1 = 0.f;
#pragma unroll 8
        for (int i = 0; i < B; ++i) {
            const float d0 = o[2 * i], d1 = o[2 * i + 1];
            const float xv = xr[(size_t)i * K + k];
            g0 = fmaf(d0, xv, g0), g1 = fmaf(d1, xv, g1);
            if (dx) dx[(size_t)i * K + k] = fmaf(d0, w0, d1 * w1);
        }
        dW[k] = g0, dW[K + k] = g1;
    }
    if (tid < 2) {
        float g = 0.f;
        for (int i = 0; i < B; ++i) g += o[2 * i + tid];
        db[tid] = g;
    }
    TAIL_STAMP(12)   // dW, db, dx
}

// The stand-alone matching loss stays in the multi-peak tail's translation unit: it is the second caller of match_assign_sample<8>,
// with run-time max_K and assignment output.  Alone with the tail, whose call passes constants, the compiler specialises that
// function for them before it is inlined, and the code of mvm_fc_head_match_step_kernel<8> comes out different.
// a 256-thread workgroup takes 256 / maxK^2 samples (16 at max_K = 4)
__global__ void __launch_bounds__(256) vm_match_loss_kernel(const float *__restrict__ mu, const float *__restrict__ kappa,
                                                            const float *__restrict__ w, const float *__restrict__ vm_gt,
                                                            const int32_t *__restrict__ K_gt, int B, int maxK, int spb,
                                                            float *__restrict__ loss_vec, float *__restrict__ dmu,
                                                            float *__restrict__ dkappa, float *__restrict__ dw,
                                                            int32_t *__restrict__ assign) {
    __shared__ float tab[3][256];   // cost, gmu, gk: [sample in block][i][j]
    const int kk = maxK * maxK, b0 = blockIdx.x * spb, tid = threadIdx.x;
    if (tid < spb * kk) {
        const int s = tid / kk, ij = tid - s * kk, i = ij / maxK, j = ij - i * maxK, b = b0 + s;
        if (b < B) {
            const int K = min(K_gt[b], maxK);
            if (i < K && j < K)
                match_cost_entry(mu[(size_t)b * maxK + i], kappa[(size_t)b * maxK + i], vm_gt[((size_t)b * maxK + j) * 3],
                                 vm_gt[((size_t)b * maxK + j) * 3 + 1], tab[0][tid], tab[1][tid], tab[2][tid]);
        }
    }
    __syncthreads();
    if (tid < spb && b0 + tid < B) {
        const int b = b0 + tid;
        const size_t o = (size_t)b * maxK;
        match_assign_sample<MATCH_KMAX>(&tab[0][tid * kk], &tab[1][tid * kk], &tab[2][tid * kk], w + o, K_gt[b], maxK, loss_vec + b, dmu ? dmu + o : nullptr,
                            dkappa ? dkappa + o : nullptr, dw ? dw + o : nullptr, assign ? assign + o : nullptr);
    }
}

// The whole tail of the multi-peak training step in ONE single-workgroup launch (round 4): the three output heads
// o = x [W_pi; W_mu; W_kappa]^T + b (models/pointnet_pp_mvM.py:91-96), the head activations (:91-125), match_loss
// (train_multi_peaks_vonMises_KL.py:54-81), its batch mean (:229) and their backward -- d loss / d W, d b of the three heads and d x.
// x: (B, K) features; the heads' weights are (KC x K), (2 KC x K), (KC x K).  In eager PyTorch terms: three Linears, the head, the loss, a
// mean and a dozen autograd nodes; as separate launches of this library: 3 x fc_small_fwd, mvm_head, vm_match_loss, torch's mean and
// its backward, three elementwise multiplies, mvm_head_bwd, 3 x fc_small_bwd.  Per-sample arithmetic is that of the standalone kernels
// (the same device functions, float32 values at the same places); the mean is a fixed-order float64 tree.  Workgroups 1 .. carry the
// next step's centre draw, as in vm_fc_head_kl_step_kernel.
template <int KC>
__global__ void __launch_bounds__(256)
mvm_fc_head_match_step_kernel(const float *__restrict__ x, const float *__restrict__ Wpi, const float *__restrict__ bpi,
                              const float *__restrict__ Wmu, const float *__restrict__ bmu, const float *__restrict__ Wkap,
                              const float *__restrict__ bkap, const float *__restrict__ vm_gt, const int32_t *__restrict__ K_gt, int B,
                              int K, float temp, float kappa_max, float *__restrict__ loss_mean, float *__restrict__ dWpi,
                              float *__restrict__ dbpi, float *__restrict__ dWmu, float *__restrict__ dbmu, float *__restrict__ dWkap,
                              float *__restrict__ dbkap, float *__restrict__ dx, float *__restrict__ mu_out, float *__restrict__ kappa_out,
                              float *__restrict__ weight_out, const SampleJob J) {
    constexpr int NO = 4 * KC;   // outputs per sample: pi (KC) | mu (2 KC) | kappa (KC)
    extern __shared__ __attribute__((aligned(16))) float sm[];   // o[B][NO] (then d_o in place), ws[NO][K], xs[B][K]
    if (blockIdx.x > 0) {
        __shared__ int nc_s;
        sample_random_body(J.seed_lo, J.seed_hi, J.str_lo, J.str_hi, J.str_dev, J.N1, J.npoint1, J.out1, J.B, J.N2, J.npoint2, J.out2,
                           (int)blockIdx.x - 1, (int)gridDim.x - 1, reinterpret_cast<unsigned long long *>(sm), nc_s);
        return;
    }
    __shared__ double red[256];
    float *o = sm;
    float *ws = sm + (((size_t)B * NO + 3) & ~(size_t)3);
    float *xs = ws + (size_t)NO * K;
    const int tid = threadIdx.x;
#ifdef PNPP_STAMPS
    unsigned long long st_last = __builtin_amdgcn_s_memtime();
#endif
    // one round trip for everything the kernel reads: the heads' weight rows in output order, their biases, the features
    for (int f = tid; f < NO * K; f += 256) {   // (the address is selected, not the loaded value: one unconditional load per element)
        const int n = f / K, k = f - n * K;
        const float *src = n < KC ? Wpi + (size_t)n * K + k : n < 3 * KC ? Wmu + (size_t)(n - KC) * K + k : Wkap + (size_t)(n - 3 * KC) * K + k;
        ws[f] = *src;
    }
    float bias_n = 0.f;
    if (tid < NO) bias_n = tid < KC ? bpi[tid] : tid < 3 * KC ? bmu[tid - KC] : bkap[tid - 3 * KC];
    {
        const int n4 = (B * K) >> 2;
        for (int f = tid; f < n4; f += 256) reinterpret_cast<float4 *>(xs)[f] = reinterpret_cast<const float4 *>(x)[f];
    }
    __shared__ float bias_s[NO];
    if (tid < NO) bias_s[tid] = bias_n;
    __syncthreads();
    TAIL_STAMP(0)   // staging
    // 1. o = x W^T + b: eight lanes per row, each a strided eighth of the features, NO accumulators per lane
    const int part8 = tid & 7;
    for (int i = tid >> 3; i < ((B + 31) & ~31); i += 32) {
        const int ic = min(i, B - 1);
        float acc[NO];
#pragma unroll
        for (int n = 0; n < NO; ++n) acc[n] = 0.f;
        for (int k = part8; k < K; k += 8) {
            const float xv = xs[(size_t)ic * K + k];
#pragma unroll
            for (int n = 0; n < NO; ++n) acc[n] = fmaf(xv, ws[n * K + k], acc[n]);
        }
#pragma unroll
        for (int n = 0; n < NO; ++n) {
#pragma unroll
            for (int m = 4; m >= 1; m >>= 1) acc[n] += __shfl_xor(acc[n], m);
            if (part8 == 0 && i < B) o[(size_t)i * NO + n] = acc[n] + bias_s[n];
        }
    }
    __syncthreads();
    // 2. head (one thread per sample), the K x K cost matrices (one thread per ENTRY: match_cost_entry), then per sample the assignment,
    // the mean's factor 1 / B (a float32 multiply, as autograd applies it) and the head's backward; d loss / d o overwrites o.
    // Tables in LDS, reusing nothing the other steps read: hm[B][3 KC] = mu | kappa | weight, tb[3][B][KC^2] = cost | gmu | gk.
    TAIL_STAMP(1)   // o = x W^T
    float *hm = xs + (size_t)B * K;
    float *tb = hm + (size_t)B * 3 * KC;
    const float gf = 1.0f / (float)B;
    for (int b = tid; b < B; b += 256) {
        const float *raw = o + (size_t)b * NO;
        mvm_head_sample(raw, raw + KC, raw + 3 * KC, KC, temp, kappa_max, hm + (size_t)b * 3 * KC, hm + (size_t)b * 3 * KC + KC,
                        hm + (size_t)b * 3 * KC + 2 * KC);
    }
    __syncthreads();
    TAIL_STAMP(2)   // head forward
    for (int e = tid; e < B * KC * KC; e += 256) {
        const int b = e / (KC * KC), ij = e - b * (KC * KC), i = ij / KC, j = ij - i * KC;
        const int Kb = min(K_gt[b], KC);
        if (i < Kb && j < Kb)
            match_cost_entry(hm[(size_t)b * 3 * KC + i], hm[(size_t)b * 3 * KC + KC + i], vm_gt[((size_t)b * KC + j) * 3],
                             vm_gt[((size_t)b * KC + j) * 3 + 1], tb[e], tb[(size_t)B * KC * KC + e], tb[(size_t)2 * B * KC * KC + e]);
    }
    __syncthreads();
    TAIL_STAMP(3)   // cost entries
    double part = 0.0;
    for (int b = tid; b < B; b += 256) {
        float raw[NO], dmu[KC], dk[KC], dw[KC], lv;
#pragma unroll
        for (int n = 0; n < NO; ++n) raw[n] = o[(size_t)b * NO + n];
        const float *mu = hm + (size_t)b * 3 * KC, *kap = mu + KC, *wt = mu + 2 * KC;
        match_assign_sample<KC>(tb + (size_t)b * KC * KC, tb + (size_t)(B + b) * KC * KC, tb + (size_t)(2 * B + b) * KC * KC, wt, K_gt[b], KC, &lv,
                            dmu, dk, dw, nullptr);
        part += (double)lv;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (mu_out) mu_out[(size_t)b * KC + k] = mu[k], kappa_out[(size_t)b * KC + k] = kap[k], weight_out[(size_t)b * KC + k] = wt[k];
            dmu[k] *= gf, dk[k] *= gf, dw[k] *= gf;
        }
        float d[NO];
        mvm_head_bwd_sample(raw + KC, raw + 3 * KC, wt, dmu, dk, dw, KC, temp, kappa_max, d, d + KC, d + 3 * KC);
#pragma unroll
        for (int n = 0; n < NO; ++n) o[(size_t)b * NO + n] = d[n];
    }
    red[tid] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) *loss_mean = (float)(red[0] / (double)B);
    TAIL_STAMP(4)   // assignment + head backward + mean
    // 3. dW = d_o^T x, db = column sums of d_o, dx = d_o W: one thread per feature, rows in order
    for (int k = tid; k < K; k += 256) {
        float wv[NO], g[NO];
#pragma unroll
        for (int n = 0; n < NO; ++n) wv[n] = ws[n * K + k], g[n] = 0.f;
        for (int i = 0; i < B; ++i) {
            const float xv = xs[(size_t)i * K + k];
            float dxv = 0.f;
#pragma unroll
            for (int n = 0; n < NO; ++n) {
                const float dn = o[(size_t)i * NO + n];
                g[n] = fmaf(dn, xv, g[n]);
                dxv = fmaf(dn, wv[n], dxv);
            }
            if (dx) dx[(size_t)i * K + k] = dxv;
        }
#pragma unroll
        for (int n = 0; n < NO; ++n) {
            float *dst = n < KC ? dWpi + (size_t)n * K : n < 3 * KC ? dWmu + (size_t)(n - KC) * K : dWkap + (size_t)(n - 3 * KC) * K;
            dst[k] = g[n];
        }
    }
    if (tid < NO) {
        float gsum = 0.f;
        for (int i = 0; i < B; ++i) gsum += o[(size_t)i * NO + tid];
        float *dst = tid < KC ? dbpi + tid : tid < 3 * KC ? dbmu + (tid - KC) : dbkap + (tid - 3 * KC);
        *dst = gsum;
    }
    TAIL_STAMP(5)   // dW, db, dx
}

}  // namespace pnpp

using namespace pnpp;

// The sampler arguments of a tail entry, those of pnpp_sample_random_dev2: the next step's centre draw (sampling.CentreRing).
struct Rider {
    uint64_t seed;
    uint64_t *stream_id_dev;
    uint64_t offset;
    int Bs, N1, npoint1;
    int32_t *out1;
    int N2, npoint2;
    int32_t *out2;
    int Nmax() const { return N1 > N2 ? N1 : N2; }
};

// Lets the draw ride in a tail's launch: validates it (null_msg, size_msg: the entry's own words; the range check speaks as
// pnpp_sample_random_dev2 does), fills the kernel's SampleJob, raises the launch's LDS to the sampling workgroups' candidate table and
// sets the grid: the tail's workgroup and 2 Bs sampling ones.
static int place_rider(const Rider &r, const char *null_msg, const char *size_msg, SampleJob &J, size_t &lds, int &grid) {
    PNPP_REQUIRE(r.stream_id_dev && r.out1 && r.out2, PNPP_ERR_ARG, "%s", null_msg);
    PNPP_REQUIRE(r.Bs > 0 && r.N1 > 0 && r.npoint1 > 0 && r.N2 > 0 && r.npoint2 > 0, PNPP_ERR_ARG, "%s", size_msg);
    PNPP_REQUIRE(r.npoint1 <= r.N1 && r.npoint2 <= r.N2, PNPP_ERR_RANGE, "sample_random_dev2: npoint exceeds N");
    const size_t lds_s = (size_t)(r.Nmax() + 1) * sizeof(unsigned long long);
    if (lds_s > lds) lds = lds_s;
    J.seed_lo = (unsigned)r.seed, J.seed_hi = (unsigned)(r.seed >> 32), J.str_lo = (unsigned)r.offset, J.str_hi = (unsigned)(r.offset >> 32);
    J.str_dev = reinterpret_cast<unsigned long long *>(r.stream_id_dev);
    J.B = r.Bs, J.N1 = r.N1, J.npoint1 = r.npoint1, J.N2 = r.N2, J.npoint2 = r.npoint2, J.out1 = r.out1, J.out2 = r.out2;
    grid = 1 + 2 * r.Bs;
    return PNPP_OK;
}

// The single-peak tail, with the next step's centre draw in its launch (rider) or without (null).  who: the entry's name in messages.
static int vm_fc_head_kl_step(const char *who, const float *x, const float *w, const float *b, const float *mu_gt, const float *kappa_gt,
                              int B, int K, float *loss_mean, float *dw, float *db, float *dx, const Rider *rider, void *stream) {
    PNPP_REQUIRE(x && w && b && mu_gt && kappa_gt && loss_mean && dw && db, PNPP_ERR_ARG, "%s: null pointer", who);
    PNPP_REQUIRE(B > 0 && K > 0 && B <= 8192, PNPP_ERR_ARG, "%s: B must be in 1..8192 and K positive", who);
    const size_t o_floats = ((size_t)2 * B + 3) & ~(size_t)3;
    const int x_in_lds = ((size_t)B * K <= 12288 && (((size_t)B * K) & 3) == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;  // <= 48 KB
    const size_t w_floats = ((size_t)2 * K + 3) & ~(size_t)3;
    size_t lds = (o_floats + w_floats + (x_in_lds ? (size_t)B * K : 0)) * sizeof(float);
    SampleJob J;
    int grid = 1;
    // fc3's two weight rows and the B x 2 outputs live in LDS beside ~7 KB of static arrays; the 64 KB a launch gets without
    // an opt-in bounds B and K together (the reference head: K = 256).  Wider heads take pnpp_fc_forward + pnpp_vm_head_kl_mean.
    if (rider) {
        PNPP_TRY(place_rider(*rider, "vm_fc_head_kl_step_sample: null sampler pointer", "vm_fc_head_kl_step_sample: non-positive sampler size",
                             J, lds, grid));
        PNPP_REQUIRE(lds <= 56 * 1024, PNPP_ERR_RANGE, "%s: %zu bytes of LDS exceed 56 KB (B=%d, K=%d, N=%d)", who, lds, B, K, rider->Nmax());
    }
    PNPP_REQUIRE(lds <= 56 * 1024, PNPP_ERR_RANGE, "%s: 2*B + 2*K (+ B*K) floats = %zu bytes of LDS exceed 56 KB (B=%d, K=%d)", who, lds, B, K);
    std::optional<ProfScope> ps;   // the launch is tagged where a draw rides in it
    if (rider)
        ps.emplace(as_stream(stream), "vm_fc_head_kl_step_kernel B=%d K=%d + sample_random B=%d N=%d npoint=%d + N=%d npoint=%d", B, K,
                   rider->Bs, rider->N1, rider->npoint1, rider->N2, rider->npoint2);
    hipLaunchKernelGGL(vm_fc_head_kl_step_kernel, dim3(grid), dim3(256), lds, as_stream(stream), x, w, b, mu_gt, kappa_gt, B, K, x_in_lds,
                       loss_mean, dw, db, dx, J);
    PNPP_CHECK_LAUNCH(who);
    return PNPP_OK;
}

extern "C" int pnpp_vm_fc_head_kl_step(const float *x, const float *w, const float *b, const float *mu_gt, const float *kappa_gt, int B,
                                       int K, float *loss_mean, float *dw, float *db, float *dx, void *stream) {
    return vm_fc_head_kl_step("vm_fc_head_kl_step", x, w, b, mu_gt, kappa_gt, B, K, loss_mean, dw, db, dx, nullptr, stream);
}

extern "C" int pnpp_vm_fc_head_kl_step_sample(const float *x, const float *w, const float *b, const float *mu_gt, const float *kappa_gt,
                                              int B, int K, float *loss_mean, float *dw, float *db, float *dx, uint64_t seed,
                                              uint64_t *stream_id_dev, uint64_t offset, int Bs, int N1, int npoint1, int32_t *out1, int N2,
                                              int npoint2, int32_t *out2, void *stream) {
    const Rider rider{seed, stream_id_dev, offset, Bs, N1, npoint1, out1, N2, npoint2, out2};
    return vm_fc_head_kl_step("vm_fc_head_kl_step_sample", x, w, b, mu_gt, kappa_gt, B, K, loss_mean, dw, db, dx, &rider, stream);
}

extern "C" int pnpp_vm_match_loss(const float *mu, const float *kappa, const float *w, const float *vm_gt,
                                  const int32_t *K_gt, int B, int maxK, float *loss_vec, float *dmu, float *dkappa, float *dw,
                                  int32_t *assign, void *stream) {
    PNPP_REQUIRE(mu && kappa && w && vm_gt && K_gt && loss_vec, PNPP_ERR_ARG, "vm_match_loss: null pointer");
    PNPP_REQUIRE(B > 0 && maxK > 0, PNPP_ERR_ARG, "vm_match_loss: non-positive size");
    PNPP_REQUIRE(maxK <= MATCH_KMAX, PNPP_ERR_ARG, "vm_match_loss: max_K=%d exceeds the supported maximum %d", maxK, MATCH_KMAX);
    const int spb = 256 / (maxK * maxK);   // samples per workgroup: one thread per cost-matrix entry
    hipLaunchKernelGGL(vm_match_loss_kernel, dim3(cdiv(B, spb)), dim3(256), 0, as_stream(stream), mu, kappa, w, vm_gt, K_gt, B,
                       maxK, spb, loss_vec, dmu, dkappa, dw, assign);
    PNPP_CHECK_LAUNCH("vm_match_loss");
    return PNPP_OK;
}

extern "C" int pnpp_mvm_fc_head_match_step(const float *x, const float *w_pi, const float *b_pi, const float *w_mu, const float *b_mu,
                                           const float *w_kappa, const float *b_kappa, const float *vm_gt, const int32_t *K_gt, int B, int K,
                                           int maxK, float temp, float kappa_max, float *loss_mean, float *dw_pi, float *db_pi, float *dw_mu,
                                           float *db_mu, float *dw_kappa, float *db_kappa, float *dx, float *mu, float *kappa, float *weight,
                                           uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int Bs, int N1, int npoint1,
                                           int32_t *out1, int N2, int npoint2, int32_t *out2, void *stream) {
    PNPP_REQUIRE(x && w_pi && b_pi && w_mu && b_mu && w_kappa && b_kappa && vm_gt && K_gt && loss_mean && dw_pi && db_pi && dw_mu && db_mu &&
                     dw_kappa && db_kappa,
                 PNPP_ERR_ARG, "mvm_fc_head_match_step: null pointer");
    PNPP_REQUIRE(B > 0 && K > 0 && (K & 3) == 0 && ((uintptr_t)x & 15) == 0, PNPP_ERR_ARG,
                 "mvm_fc_head_match_step: B must be positive, K a positive multiple of 4, x 16-byte aligned");
    PNPP_REQUIRE(maxK == 4 || maxK == 8, PNPP_ERR_ARG, "mvm_fc_head_match_step: max_K must be 4 or 8 (got %d); other widths take the separate launches", maxK);
    PNPP_REQUIRE(!mu || (kappa && weight), PNPP_ERR_ARG, "mvm_fc_head_match_step: mu, kappa, weight come together");
    const int NO = 4 * maxK;
    // o[B][NO] | ws[NO][K] | xs[B][K] | mu, kappa, weight [B][3 max_K] | cost, gmu, gk [3][B][max_K^2]
    size_t lds = ((((size_t)B * NO + 3) & ~(size_t)3) + (size_t)NO * K + (size_t)B * K + (size_t)B * 3 * maxK + (size_t)3 * B * maxK * maxK) *
                 sizeof(float);
    SampleJob J;
    int grid = 1;
    if (Bs > 0) {   // the next step's centre draw rides in this launch (sampling.CentreRing)
        const Rider rider{seed, stream_id_dev, offset, Bs, N1, npoint1, out1, N2, npoint2, out2};
        const char *bad = "mvm_fc_head_match_step: bad sampler arguments";
        PNPP_TRY(place_rider(rider, bad, bad, J, lds, grid));
    }
    // features, the 4 max_K weight rows, the outputs and the match tables live in LDS (the reference head, B = 32: 59 KB)
    PNPP_REQUIRE(lds <= 96 * 1024, PNPP_ERR_RANGE, "mvm_fc_head_match_step: %zu bytes of LDS exceed 96 KB (B=%d, K=%d, max_K=%d)", lds, B, K, maxK);
    {   // more than the 64 KB a launch gets without asking
        static bool granted[2] = {false, false};
        const int which = maxK == 4 ? 0 : 1;
        if (!granted[which]) {
            const void *fn = maxK == 4 ? (const void *)mvm_fc_head_match_step_kernel<4> : (const void *)mvm_fc_head_match_step_kernel<8>;
            (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
            granted[which] = true;
        }
    }
    ProfScope ps(as_stream(stream), "mvm_fc_head_match_step_kernel B=%d K=%d maxK=%d%s", B, K, maxK, Bs > 0 ? " + sample_random" : "");
    if (maxK == 4) {
        hipLaunchKernelGGL(mvm_fc_head_match_step_kernel<4>, dim3(grid), dim3(256), lds, as_stream(stream), x, w_pi, b_pi, w_mu, b_mu, w_kappa,
                           b_kappa, vm_gt, K_gt, B, K, temp, kappa_max, loss_mean, dw_pi, db_pi, dw_mu, db_mu, dw_kappa, db_kappa, dx, mu, kappa,
                           weight, J);
    } else {
        hipLaunchKernelGGL(mvm_fc_head_match_step_kernel<8>, dim3(grid), dim3(256), lds, as_stream(stream), x, w_pi, b_pi, w_mu, b_mu, w_kappa,
                           b_kappa, vm_gt, K_gt, B, K, temp, kappa_max, loss_mean, dw_pi, db_pi, dw_mu, db_mu, dw_kappa, db_kappa, dx, mu, kappa,
                           weight, J);
    }
    PNPP_CHECK_LAUNCH("mvm_fc_head_match_step");
    return PNPP_OK;
}

#ifdef PNPP_STAMPS
extern "C" int pnpp_debug_tail_stamps(unsigned long long *out16, int reset) {
    if (reset) {
        unsigned long long z[16] = {0};
        hipMemcpyToSymbol(HIP_SYMBOL(pnpp::g_tail_stamps), z, sizeof(z));
    } else {
        hipDeviceSynchronize();
        hipMemcpyFromSymbol(out16, HIP_SYMBOL(pnpp::g_tail_stamps), 16 * sizeof(unsigned long long));
    }
    return 0;
}
#endif
