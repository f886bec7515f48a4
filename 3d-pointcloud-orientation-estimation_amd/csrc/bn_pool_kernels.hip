// bn_pool_kernels.hip -- what runs between the GEMMs of a level: the fixed-order reductions of the dW and statistics slabs, the BatchNorm
// finalisation forward and backward (with the dZ materialisation and the slab reduction that ride in its launch: post_gemm), and the
// max-pooling over the neighbourhood forward and backward.
#include "launch.h"
#include "split_prims.h"

namespace pnpp {

// out[c][perm(k)] = sum_s slab[s][c][k], fixed summation order: block = EPB outputs x (256/EPB) split lanes,
// every lane strides the splits with four independent partial sums, the lanes are combined in lane order.
// Small outputs (a 64 x 3 weight) take 16 outputs per block so that the splits, not the outputs, fill the chip.
template <int EPB>
__device__ __forceinline__ void slab_reduce_block(const SlabReduceArgs &R, int bid) {
    constexpr int SL = 256 / EPB;
    __shared__ float red[SL][EPB];
    const int total = R.Nc * R.Kvalid;
    const int e = threadIdx.x % EPB, sl = threadIdx.x / EPB;
    const int i = bid * EPB + e;
    float acc = 0.f;
    int c = 0, k = 0;
    if (i < total) {
        c = i / R.Kvalid, k = i - c * R.Kvalid;
        const float *p = R.slab + (size_t)c * R.kp_pad + k;
        const size_t stride = (size_t)R.Nc * R.kp_pad;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int s = sl;
        for (; s + 3 * SL < R.nsplit; s += 4 * SL) {
            a0 += p[(size_t)s * stride];
            a1 += p[(size_t)(s + SL) * stride];
            a2 += p[(size_t)(s + 2 * SL) * stride];
            a3 += p[(size_t)(s + 3 * SL) * stride];
        }
        for (; s < R.nsplit; s += SL) a0 += p[(size_t)s * stride];
        acc = (a0 + a1) + (a2 + a3);
    }
    red[sl][e] = acc;
    __syncthreads();
    if (sl == 0 && i < total) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < SL; ++j) t += red[j][e];
        int ko = k;
        if (R.perm_D >= 0) ko = k < R.perm_D ? k + 3 : k - R.perm_D;  // features-first -> xyz-first (state_dict order)
        R.out[(size_t)c * R.ldo + ko] = t;
    }
}

// the same reduction on groups of four consecutive k (16-byte loads and stores, a quarter of the threads and load
// instructions): block = EPB groups x (256/EPB) split lanes.  Needs Kvalid, kp_pad, ldo multiples of 4, no permutation.
template <int EPB>
__device__ __forceinline__ void slab_reduce_block4(const SlabReduceArgs &R, int bid) {
    constexpr int SL = 256 / EPB;
    __shared__ float4 red4[SL][EPB];
    const int kg = R.Kvalid >> 2, total = R.Nc * kg;
    const int e = threadIdx.x % EPB, sl = threadIdx.x / EPB;
    const int i = bid * EPB + e;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int c = 0, k = 0;
    if (i < total) {
        c = i / kg, k = 4 * (i - c * kg);
        const float *p = R.slab + (size_t)c * R.kp_pad + k;
        const size_t stride = (size_t)R.Nc * R.kp_pad;
        float4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        int s = sl;
        for (; s + 3 * SL < R.nsplit; s += 4 * SL) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 q = *reinterpret_cast<const float4 *>(p + (size_t)(s + u * SL) * stride);
                a[u].x += q.x, a[u].y += q.y, a[u].z += q.z, a[u].w += q.w;
            }
        }
        for (; s < R.nsplit; s += SL) {
            const float4 q = *reinterpret_cast<const float4 *>(p + (size_t)s * stride);
            a[0].x += q.x, a[0].y += q.y, a[0].z += q.z, a[0].w += q.w;
        }
        acc = make_float4((a[0].x + a[1].x) + (a[2].x + a[3].x), (a[0].y + a[1].y) + (a[2].y + a[3].y),
                          (a[0].z + a[1].z) + (a[2].z + a[3].z), (a[0].w + a[1].w) + (a[2].w + a[3].w));
    }
    red4[sl][e] = acc;
    __syncthreads();
    if (sl == 0 && i < total) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < SL; ++j) {
            const float4 q = red4[j][e];
            t.x += q.x, t.y += q.y, t.z += q.z, t.w += q.w;
        }
        *reinterpret_cast<float4 *>(R.out + (size_t)c * R.ldo + k) = t;
    }
}

static inline bool slab_reduce_vec4(const SlabReduceArgs &R) {  // few, wide partials (measured: no gain once nsplit > 32)
    return R.nsplit <= 32 && R.perm_D < 0 && (R.Kvalid & 3) == 0 && (R.kp_pad & 3) == 0 && (R.ldo & 3) == 0 && (((uintptr_t)R.slab | (uintptr_t)R.out) & 15) == 0;
}
// groups per block for the 16-byte form: few splits -> many groups per block; many splits -> many split lanes
static inline int slab_reduce_epb4(int nsplit) { return nsplit <= 32 ? 64 : nsplit <= 128 ? 16 : 4; }

template <int EPB, bool V4 = false>
__global__ void __launch_bounds__(256) slab_reduce_kernel(SlabReduceArgs R) {
    if constexpr (V4) slab_reduce_block4<EPB>(R, blockIdx.x);
    else slab_reduce_block<EPB>(R, blockIdx.x);
}

static inline bool slab_reduce_wide(int total, int nsplit) { return total >= 16384 || nsplit <= 8; }

// two independent reductions in one launch (scalar form): blocks [0, n1) take R1, the rest R2
template <int EPB1, int EPB2>
__global__ void __launch_bounds__(256) slab_reduce2_kernel(SlabReduceArgs R1, int n1, SlabReduceArgs R2) {
    if ((int)blockIdx.x < n1) slab_reduce_block<EPB1>(R1, blockIdx.x);
    else slab_reduce_block<EPB2>(R2, blockIdx.x - n1);
}

// the blocks of the two-reduction launch and the form it takes (wide: 64 outputs per block, else 16)
static inline void slab_reduce2_plan(const SlabReduceArgs &R1, const SlabReduceArgs &R2, bool *w1, bool *w2, int *n1, int *n2) {
    const int t1 = R1.Nc * R1.Kvalid, t2 = R2.Nc * R2.Kvalid;
    *w1 = slab_reduce_wide(t1, R1.nsplit), *w2 = slab_reduce_wide(t2, R2.nsplit);
    *n1 = cdiv(t1, *w1 ? 64 : 16), *n2 = cdiv(t2, *w2 ? 64 : 16);
}

static int launch_slab_reduce2(const SlabReduceArgs &R1, const SlabReduceArgs &R2, hipStream_t st) {
    bool w1, w2;
    int n1, n2;
    slab_reduce2_plan(R1, R2, &w1, &w2, &n1, &n2);
    ProfScope ps(st, "slab_reduce2_kernel N=%d K=%d split=%d | N=%d K=%d split=%d", R1.Nc, R1.Kvalid, R1.nsplit, R2.Nc, R2.Kvalid, R2.nsplit);
    if (w1 && w2) hipLaunchKernelGGL((slab_reduce2_kernel<64, 64>), dim3(n1 + n2), dim3(256), 0, st, R1, n1, R2);
    else if (w1) hipLaunchKernelGGL((slab_reduce2_kernel<64, 16>), dim3(n1 + n2), dim3(256), 0, st, R1, n1, R2);
    else if (w2) hipLaunchKernelGGL((slab_reduce2_kernel<16, 64>), dim3(n1 + n2), dim3(256), 0, st, R1, n1, R2);
    else hipLaunchKernelGGL((slab_reduce2_kernel<16, 16>), dim3(n1 + n2), dim3(256), 0, st, R1, n1, R2);
    PNPP_CHECK_LAUNCH("slab_reduce2");
    return PNPP_OK;
}
int launch_slab_reduce2(const float *slab1, int nsplit1, int Nc1, int kp_pad1, int Kvalid1, float *out1, int ldo1, const float *slab2,
                        int nsplit2, int Nc2, int kp_pad2, int Kvalid2, float *out2, int ldo2, hipStream_t st) {
    const SlabReduceArgs R1{slab1, nsplit1, Nc1, kp_pad1, Kvalid1, -1, out1, ldo1}, R2{slab2, nsplit2, Nc2, kp_pad2, Kvalid2, -1, out2, ldo2};
    return launch_slab_reduce2(R1, R2, st);
}

static int launch_slab_reduce(const SlabReduceArgs &R, hipStream_t st) {
    const int total = R.Nc * R.Kvalid, nsplit = R.nsplit;
    ProfScope ps(st, "slab_reduce_kernel N=%d K=%d split=%d", R.Nc, R.Kvalid, nsplit);
    if (slab_reduce_vec4(R)) {
        const int groups = total / 4, epb = slab_reduce_epb4(nsplit);
        if (epb == 64) hipLaunchKernelGGL((slab_reduce_kernel<64, true>), dim3(cdiv(groups, 64)), dim3(256), 0, st, R);
        else if (epb == 16) hipLaunchKernelGGL((slab_reduce_kernel<16, true>), dim3(cdiv(groups, 16)), dim3(256), 0, st, R);
        else hipLaunchKernelGGL((slab_reduce_kernel<4, true>), dim3(cdiv(groups, 4)), dim3(256), 0, st, R);
    } else if (slab_reduce_wide(total, nsplit))
        hipLaunchKernelGGL(slab_reduce_kernel<64>, dim3(cdiv(total, 64)), dim3(256), 0, st, R);
    else
        hipLaunchKernelGGL(slab_reduce_kernel<16>, dim3(cdiv(total, 16)), dim3(256), 0, st, R);
    PNPP_CHECK_LAUNCH("slab_reduce");
    return PNPP_OK;
}
int launch_slab_reduce(const float *slab, int nsplit, int Nc, int kp_pad, int Kvalid, int perm_D, float *out, int ldo,
                       hipStream_t st) {
    return launch_slab_reduce(SlabReduceArgs{slab, nsplit, Nc, kp_pad, Kvalid, perm_D, out, ldo}, st);
}

// ---- a level's trailing reduction handed on (SaTail, kernels.h) ----
// The two forms the merged pooling launch exists for are the two the training step runs: one scalar reduction at 64 outputs per
// block (layer 0 of the group_all level: permuted columns), and the <16, 64> pair of a delayed layer 0 (few coordinate outputs
// over many partials, then the wide feature block).  Every other form runs as its own launch.
static inline bool slab_tail_rides(const SaTail &T) {
    if (T.kind == PNPP_SA_TAIL_SLAB_REDUCE) return !slab_reduce_vec4(T.R1) && slab_reduce_wide(T.R1.Nc * T.R1.Kvalid, T.R1.nsplit);
    if (T.kind == PNPP_SA_TAIL_SLAB_REDUCE2) {
        bool w1, w2;
        int n1, n2;
        slab_reduce2_plan(T.R1, T.R2, &w1, &w2, &n1, &n2);
        return !w1 && w2;
    }
    return false;
}

int slab_tail_blocks(const SaTail &T) {
    if (T.kind == PNPP_SA_TAIL_SLAB_REDUCE) {
        const int total = T.R1.Nc * T.R1.Kvalid;
        if (slab_reduce_vec4(T.R1)) return cdiv(total / 4, slab_reduce_epb4(T.R1.nsplit));
        return cdiv(total, slab_reduce_wide(total, T.R1.nsplit) ? 64 : 16);
    }
    if (T.kind == PNPP_SA_TAIL_SLAB_REDUCE2) {
        bool w1, w2;
        int n1, n2;
        slab_reduce2_plan(T.R1, T.R2, &w1, &w2, &n1, &n2);
        return n1 + n2;
    }
    return 0;
}

int launch_slab_tail(const SaTail &T, hipStream_t st) {
    if (T.kind == PNPP_SA_TAIL_SLAB_REDUCE) return launch_slab_reduce(T.R1, st);
    if (T.kind == PNPP_SA_TAIL_SLAB_REDUCE2) return launch_slab_reduce2(T.R1, T.R2, st);
    PNPP_REQUIRE(T.kind == PNPP_SA_TAIL_NONE, PNPP_ERR_ARG, "sa tail: unknown kind %d", T.kind);
    return PNPP_OK;
}

// ---------------------------------------------------------------------------------------------
// BatchNorm statistics finalisation (float64 reduction of the slab partials, fixed order)
// block = 8 columns x 32 slab lanes (each lane owns every 32nd slab; fixed-order tree afterwards)
constexpr int FIN_COLS = 8;
__device__ __forceinline__ void slab_column_sums(const double *__restrict__ slab, int nslab, int C, int c, double &o1,
                                                 double &o2, double (*red)[2][FIN_COLS]) {
    const int g = threadIdx.x / FIN_COLS, cl = threadIdx.x % FIN_COLS;
    double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0;
    if (c < C) {
        int s = g;
#pragma unroll 4  // 16 independent loads in flight per lane: the reduction is a chain of L2 round trips otherwise
        for (; s + 32 < nslab; s += 64) {
            a0 += slab[((size_t)s * 2 + 0) * C + c];
            b0 += slab[((size_t)s * 2 + 1) * C + c];
            a1 += slab[((size_t)(s + 32) * 2 + 0) * C + c];
            b1 += slab[((size_t)(s + 32) * 2 + 1) * C + c];
        }
        for (; s < nslab; s += 32) {
            a0 += slab[((size_t)s * 2 + 0) * C + c];
            b0 += slab[((size_t)s * 2 + 1) * C + c];
        }
    }
    red[g][0][cl] = a0 + a1;
    red[g][1][cl] = b0 + b1;
    __syncthreads();
    o1 = 0.0, o2 = 0.0;
#pragma unroll
    for (int i = 0; i < 32; ++i) o1 += red[i][0][cl], o2 += red[i][1][cl];
}

__global__ void __launch_bounds__(256)
bn_finalize_fwd_kernel(const double *__restrict__ slab, int nslab, int C, double count, const float *__restrict__ bias,
                       const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ rm,
                       float *__restrict__ rv, long long *__restrict__ nbt, float momentum, float eps, int training,
                       float *__restrict__ mean, float *__restrict__ istd, float *__restrict__ scale,
                       float *__restrict__ shift, const double *__restrict__ count_dev, const float *__restrict__ pool_ext,
                       float *__restrict__ pool_out, int G, int32_t *__restrict__ pool_arg, float *__restrict__ origin_a,
                       float *__restrict__ origin_b, int norigin) {
    __shared__ double red[32][2][FIN_COLS];
    if (blockIdx.x == 0 && blockIdx.y == 0)   // group_all levels: every cloud's centre is the origin (pointnet_pp_8dir.py:24)
        for (int i = threadIdx.x; i < norigin; i += 256) {
            if (origin_a) origin_a[i] = 0.f;
            if (origin_b) origin_b[i] = 0.f;
        }
    __shared__ float pool_cs[2][FIN_COLS];
    if (count_dev) count = *count_dev;   // SyncBN: the row count of ALL ranks, summed with the statistics
    // pooling in the producer's epilogue (Epilogue::pool_ext): gridDim.y row blocks each redo the slab reduction for their 8
    // channels (identical sums, identical order) and turn their rows of the extreme pre-BN values into the pooled output;
    // the statistics themselves are written by row block 0 only
    const bool writer = blockIdx.y == 0;
    if (training && nbt && blockIdx.x == 0 && writer && threadIdx.x == 0) *nbt += 1;  // num_batches_tracked (nn.BatchNorm forward)
    const int c = blockIdx.x * FIN_COLS + (threadIdx.x % FIN_COLS);
    // The per-channel parameters are requested BEFORE the slab reduction: at a kernel boundary every line is a cold miss of this
    // XCD's L2 (~1.5 us), the reduction ends in a barrier the compiler will not move loads across, and a launch this short is
    // the sum of its dependent round trips -- one instead of two.
    const bool owner = threadIdx.x < FIN_COLS && c < C;
    float p_bias = 0.f, p_g = 1.f, p_b = 0.f, p_rm = 0.f, p_rv = 0.f;
    if (owner || (!training && c < C)) {
        if (bias) p_bias = bias[c];
        if (rm) p_rm = rm[c], p_rv = rv[c];
    }
    if (owner) {
        if (gamma) p_g = gamma[c];
        if (beta) p_b = beta[c];
    }
    double mu, var;
    if (training) {
        double s1, s2;
        slab_column_sums(slab, nslab, C, c, s1, s2, red);
        mu = s1 / count;
        var = s2 / count - mu * mu;
        if (var < 0.0) var = 0.0;
    } else {
        if (c >= C) return;
        // eval: normalise z + bias with the running statistics  ->  "mean" of the bias-free z is rm - bias
        mu = (double)p_rm - (double)p_bias;
        var = (double)p_rv;
    }
    if (owner) {
        const double is = 1.0 / sqrt(var + (double)eps);
        const double g = (double)p_g, bt = (double)p_b;
        const float sc = (float)(g * is), sh = (float)(bt - mu * g * is);
        if (pool_out) pool_cs[0][threadIdx.x] = sc, pool_cs[1][threadIdx.x] = sh;
        if (writer) {
            mean[c] = (float)mu;
            istd[c] = (float)is;
            scale[c] = sc;
            shift[c] = sh;
            if (training && rm) {
                const double bmean = mu + (double)p_bias;  // the conv/linear bias was folded out of z
                const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
                rm[c] = (float)((1.0 - (double)momentum) * (double)p_rm + (double)momentum * bmean);
                rv[c] = (float)((1.0 - (double)momentum) * (double)p_rv + (double)momentum * unbiased);
            }
        }
    }
    if (!pool_out) return;
    __syncthreads();
    // out[g][c] = relu(scale * ext + shift): 8 consecutive channels (32 bytes) of 32 rows per pass
    const int cl = threadIdx.x % FIN_COLS, cc = blockIdx.x * FIN_COLS + cl;
    if (cc >= C) return;
    const float sc = pool_cs[0][cl], sh = pool_cs[1][cl];
    const int rows_per = (G + gridDim.y - 1) / gridDim.y, g0 = blockIdx.y * rows_per, g1 = min(G, g0 + rows_per);
    for (int gg = g0 + threadIdx.x / FIN_COLS; gg < g1; gg += 256 / FIN_COLS) {
        const size_t i = (size_t)gg * C + cc;
        const float v = fmaf(pool_ext[i], sc, sh);
        pool_out[i] = fmaxf(v, 0.f);
        // a neighbourhood whose activations are all zero routes (no) gradient through its first row, as torch.max over the
        // post-ReLU values does -- and the backward pass then reads one z row per group instead of a scattered one
        if (pool_arg && !(v > 0.f)) pool_arg[i] = 0;
    }
}

struct BnFinalizeBwdArgs {
    const double *slab;
    int nslab, C;
    double count;
    int training;
    const float *gamma, *mean, *istd;
    float *cst, *dgamma, *dbeta, *dbias;
    // SyncBN: `slab` holds the sums over ALL ranks (one slab), *count_dev their row count; the parameter gradients stay this
    // rank's own sums (`local`: [2][C]) -- the gradient all-reduce adds the ranks up, as it does for every other parameter
    const double *count_dev = nullptr, *local = nullptr;
    // Pooled source (levels with few groups: the group_all level has one per cloud): the column sums are taken straight from the pooled
    // gradient -- sum over the G groups of d = ReLU'(scale zsel + shift) dout and of d xhat(zsel) -- instead of from slabs a pool_bwd
    // launch would have written; the dZ job rebuilds d the same way.  No pool_bwd launch, no dm tensor.
    const float *p_dout = nullptr, *p_zsel = nullptr, *p_scale = nullptr, *p_shift = nullptr;
    int p_G = 0;
};

// column sums of one channel from the pooled source, groups in order
__device__ __forceinline__ void pooled_column_sums(const BnFinalizeBwdArgs &F, int c, double &s1, double &s2) {
    const float sc = F.p_scale[c], sh = F.p_shift[c], mu = F.mean[c], is = F.istd[c];
    s1 = 0.0, s2 = 0.0;
    for (int g0 = 0; g0 < F.p_G; g0 += 8) {   // eight groups' two streams in flight at a time (all 32 at once measured the same)
        float za[8], dv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const size_t gi = (size_t)min(g0 + j, F.p_G - 1) * F.C + c;
            za[j] = F.p_zsel[gi], dv[j] = F.p_dout[gi];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = (g0 + j < F.p_G && fmaf(za[j], sc, sh) > 0.f) ? dv[j] : 0.f;
            s1 += (double)d, s2 += (double)d * (double)((za[j] - mu) * is);
        }
    }
}

__device__ __forceinline__ void bn_finalize_bwd_block(const BnFinalizeBwdArgs &F, int bid) {
    __shared__ double red[32][2][FIN_COLS];
    const int C = F.C;
    const int c = bid * FIN_COLS + (threadIdx.x % FIN_COLS);
    // (parameters first, reduction second: see bn_finalize_fwd_kernel)
    const bool owner = threadIdx.x < FIN_COLS && c < C;
    float g = 1.f, p_is = 0.f, p_mu = 0.f;
    if (owner) {
        if (F.gamma) g = F.gamma[c];
        p_is = F.istd[c], p_mu = F.mean[c];
    }
    double s1, s2;
    if (F.p_dout) {
        if (!owner) return;
        pooled_column_sums(F, c, s1, s2);
    } else {
        slab_column_sums(F.slab, F.nslab, C, c, s1, s2, red);
        if (!owner) return;
    }
    const double count = F.count_dev ? *F.count_dev : F.count;
    float *cst = F.cst;
    cst[c] = g * p_is;
    cst[C + c] = p_mu;
    cst[2 * C + c] = p_is;
    cst[3 * C + c] = F.training ? (float)(s1 / count) : 0.f;
    cst[4 * C + c] = F.training ? (float)(s2 / count) : 0.f;
    if (F.local) s1 = F.local[c], s2 = F.local[C + c];
    if (F.dgamma) F.dgamma[c] = (float)s2;
    if (F.dbeta) F.dbeta[c] = (float)s1;
    // a bias in front of a train-mode BatchNorm has exactly zero gradient; with running
    // statistics the layer is affine and d(bias) = sum_m dz = g * sum_m dy
    if (F.dbias) F.dbias[c] = F.training ? 0.f : (float)((double)(g * p_is) * s1);
}

// Small-M levels materialise dZ once per layer (dz_materialize_kernel).  The BatchNorm-backward constants it needs are
// a 32-slab column reduction, so the workgroups that write dZ redo that reduction for their own 64 columns (in their
// own fixed order: the constants can differ from `cst` in the last float32 bit, deterministically) and the materialisation rides in the launch that finalises: no
// launch of its own, no wait for `cst`.
struct DzJob {
    const float *dy = nullptr;   // masked upstream gradient (M x C), or the pooled gradient (G x C) when arg != nullptr
    const float *z = nullptr;    // pre-BN activations (M x C)
    const int32_t *arg = nullptr;  // pooled form: arg-max neighbour per (group, channel)
    int K = 1;                   // pooled form: rows per group
    int M = 0;
    float *out = nullptr;        // dZ (M x C); nullptr = no job
};

__device__ __forceinline__ void dz_fused_block(const BnFinalizeBwdArgs &F, const DzJob &J, int bid) {
    __shared__ double red[4][2][64];
    __shared__ float kc[5][64];  // g, mu, istd, c1, c2 of this block's 64 columns
    const int C = F.C, ncg = (C + 63) / 64;
    const int c0 = (bid % ncg) * 64, r0 = (bid / ncg) * 64;
    {   // column sums of the slabs: 64 columns x 4 slab lanes, every load of a lane in flight at once, lanes combined in order
        const int cl = threadIdx.x & 63, q = threadIdx.x >> 6, c = min(c0 + cl, C - 1);
        double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
        if (F.p_dout) {   // pooled source: lane 0 of the four takes the whole column (a few dozen groups)
            if (q == 0) pooled_column_sums(F, c, a1, a2);
        }
        int sidx = F.p_dout ? F.nslab : q;
#pragma unroll 4
        for (; sidx + 4 < F.nslab; sidx += 8) {
            a1 += F.slab[((size_t)sidx * 2 + 0) * C + c];
            a2 += F.slab[((size_t)sidx * 2 + 1) * C + c];
            b1 += F.slab[((size_t)(sidx + 4) * 2 + 0) * C + c];
            b2 += F.slab[((size_t)(sidx + 4) * 2 + 1) * C + c];
        }
        for (; sidx < F.nslab; sidx += 4) {
            a1 += F.slab[((size_t)sidx * 2 + 0) * C + c];
            a2 += F.slab[((size_t)sidx * 2 + 1) * C + c];
        }
        red[q][0][cl] = a1 + b1;
        red[q][1][cl] = a2 + b2;
        __syncthreads();
        if (threadIdx.x < 64) {
            const double s1 = (red[0][0][cl] + red[1][0][cl]) + (red[2][0][cl] + red[3][0][cl]);
            const double s2 = (red[0][1][cl] + red[1][1][cl]) + (red[2][1][cl] + red[3][1][cl]);
            const float g = F.gamma ? F.gamma[c] : 1.f;
            kc[0][cl] = g * F.istd[c];
            kc[1][cl] = F.mean[c];
            kc[2][cl] = F.istd[c];
            const double count = F.count_dev ? *F.count_dev : F.count;
            kc[3][cl] = F.training ? (float)(s1 / count) : 0.f;
            kc[4][cl] = F.training ? (float)(s2 / count) : 0.f;
        }
        __syncthreads();
    }
    const int q4 = 4 * (threadIdx.x & 15), c = c0 + q4;
    if (c >= C) return;
    const float4 g = *reinterpret_cast<const float4 *>(&kc[0][q4]), mu = *reinterpret_cast<const float4 *>(&kc[1][q4]);
    const float4 is = *reinterpret_cast<const float4 *>(&kc[2][q4]), c1 = *reinterpret_cast<const float4 *>(&kc[3][q4]);
    const float4 c2 = *reinterpret_cast<const float4 *>(&kc[4][q4]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = r0 + (threadIdx.x >> 4) + 16 * i;
        if (row >= J.M) continue;
        const float4 z = *reinterpret_cast<const float4 *>(J.z + (size_t)row * C + c);
        float4 dy;
        if (J.arg) {
            const int grp = row / J.K, kk = row - grp * J.K;
            float4 dm = *reinterpret_cast<const float4 *>(J.dy + (size_t)grp * C + c);
            if (F.p_dout) {   // J.dy is dout itself: d = ReLU'(scale zsel + shift) dout, as pool_bwd_kernel writes it
                const float4 zs = *reinterpret_cast<const float4 *>(F.p_zsel + (size_t)grp * C + c);
                const float4 ps = *reinterpret_cast<const float4 *>(F.p_scale + c), ph = *reinterpret_cast<const float4 *>(F.p_shift + c);
                dm.x = fmaf(zs.x, ps.x, ph.x) > 0.f ? dm.x : 0.f, dm.y = fmaf(zs.y, ps.y, ph.y) > 0.f ? dm.y : 0.f;
                dm.z = fmaf(zs.z, ps.z, ph.z) > 0.f ? dm.z : 0.f, dm.w = fmaf(zs.w, ps.w, ph.w) > 0.f ? dm.w : 0.f;
            }
            const int4 ia = *reinterpret_cast<const int4 *>(J.arg + (size_t)grp * C + c);
            dy = make_float4(kk == ia.x ? dm.x : 0.f, kk == ia.y ? dm.y : 0.f, kk == ia.z ? dm.z : 0.f, kk == ia.w ? dm.w : 0.f);
        } else {
            dy = *reinterpret_cast<const float4 *>(J.dy + (size_t)row * C + c);
        }
        float4 o;  // the operand loaders' formula (xform_a4<A_DZ>)
        o.x = g.x * (dy.x - c1.x - (z.x - mu.x) * is.x * c2.x);
        o.y = g.y * (dy.y - c1.y - (z.y - mu.y) * is.y * c2.y);
        o.z = g.z * (dy.z - c1.z - (z.z - mu.z) * is.z * c2.z);
        o.w = g.w * (dy.w - c1.w - (z.w - mu.w) * is.w * c2.w);
        *reinterpret_cast<float4 *>(J.out + (size_t)row * C + c) = o;
    }
}
static inline int dz_job_blocks(const DzJob &J, int C) { return J.out ? ((C + 63) / 64) * ((J.M + 63) / 64) : 0; }

__global__ void __launch_bounds__(256) bn_finalize_bwd_kernel(BnFinalizeBwdArgs F, int nfin, DzJob J) {
    if ((int)blockIdx.x < nfin) bn_finalize_bwd_block(F, blockIdx.x);
    else dz_fused_block(F, J, blockIdx.x - nfin);
}

// the two reductions that follow a backward GEMM -- the weight-gradient partials of layer l and the BatchNorm-backward
// column sums of layer l-1 -- share one launch: the first nfin workgroups finalise, the rest reduce slabs
template <int EPB, bool V4 = false>
__global__ void __launch_bounds__(256) post_gemm_kernel(BnFinalizeBwdArgs F, int nfin, SlabReduceArgs R, int ndz, DzJob J) {
    if ((int)blockIdx.x < nfin) bn_finalize_bwd_block(F, blockIdx.x);
    else if ((int)blockIdx.x < nfin + ndz) dz_fused_block(F, J, blockIdx.x - nfin);
    else if constexpr (V4) slab_reduce_block4<EPB>(R, blockIdx.x - nfin - ndz);
    else slab_reduce_block<EPB>(R, blockIdx.x - nfin - ndz);
}

// SyncBN: the [nslab][2][C] partials of THIS rank reduced to one [2][C] slab followed by the row count, written twice -- `glob`
// is summed over the ranks in place by the registered exchange, `local` keeps this rank's own sums for the parameter gradients
__global__ void __launch_bounds__(256)
slab_sum_kernel(const double *__restrict__ slab, int nslab, int C, double count, double *__restrict__ glob, double *__restrict__ local) {
    __shared__ double red[32][2][FIN_COLS];
    const int c = blockIdx.x * FIN_COLS + (threadIdx.x % FIN_COLS);
    double s1, s2;
    slab_column_sums(slab, nslab, C, c, s1, s2, red);
    if (threadIdx.x < FIN_COLS && c < C) {
        glob[c] = s1, glob[C + c] = s2;
        local[c] = s1, local[C + c] = s2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) glob[2 * C] = count, local[2 * C] = count;
}

int launch_slab_sum(const double *slab, int nslab, int C, double count, double *glob, double *local, hipStream_t st) {
    ProfScope ps(st, "slab_sum_kernel C=%d", C);
    hipLaunchKernelGGL(slab_sum_kernel, dim3(cdiv(C, FIN_COLS)), dim3(256), 0, st, slab, nslab, C, count, glob, local);
    PNPP_CHECK_LAUNCH("slab_sum");
    return PNPP_OK;
}

int launch_bn_finalize_fwd(const StatsView &V, double count, const BnLayer &bn, const BnHyper &h, hipStream_t st, const PoolTail *tail) {
    const PoolTail T = tail ? *tail : PoolTail();
    const bool pool = T.pool_ext && T.pool_out && T.G > 0 && h.training;
    int gy = 1, C = bn.C;
    if (pool) {   // enough row blocks to fill the chip, at least 64 rows each
        gy = cdiv(256, cdiv(C, FIN_COLS));
        if (gy > cdiv(T.G, 64)) gy = cdiv(T.G, 64);
        if (gy < 1) gy = 1;
    }
    ProfScope ps(st, "bn_finalize_fwd_kernel C=%d%s", C, pool ? " +pool" : "");
    hipLaunchKernelGGL(bn_finalize_fwd_kernel, dim3(cdiv(C, FIN_COLS), gy), dim3(256), 0, st, V.slab, V.nslab, C, count, bn.bias, bn.gamma,
                       bn.beta, bn.rm, bn.rv, bn.nbt, h.momentum, h.eps, h.training, bn.mean, bn.istd, bn.scale, bn.shift, V.count_dev,
                       pool ? T.pool_ext : nullptr, pool ? T.pool_out : nullptr, T.G, pool ? T.pool_arg : nullptr,
                       pool ? T.origin_a : nullptr, pool ? T.origin_b : nullptr, pool ? T.norigin : 0);
    PNPP_CHECK_LAUNCH("bn_finalize_fwd");
    return PNPP_OK;
}

static DzJob make_dz_job(const DzSide &S, int C) {
    DzJob J;
    const AOperand *dz = S.dz;
    if (dz && S.out && (C & 3) == 0 && dz->lda == C && (dz->mode == A_DZ || dz->mode == A_DZ_POOL)) {
        J.dy = dz->a, J.z = dz->z, J.M = S.M, J.out = S.out;
        if (dz->mode == A_DZ_POOL) J.arg = dz->arg, J.K = dz->K;
    }
    return J;
}
static BnFinalizeBwdArgs make_finalize_bwd(const StatsView &V, double count, int training, const BnLayer &bn, float *cst, const BnGrads &g) {
    return BnFinalizeBwdArgs{V.slab, V.nslab, bn.C, count, training, bn.gamma, bn.mean, bn.istd, cst, g.dgamma, g.dbeta, g.dbias, V.count_dev, V.local};
}

int launch_bn_finalize_bwd(const StatsView &V, double count, int training, const BnLayer &bn, float *cst, const BnGrads &g, hipStream_t st,
                           const DzSide &dz, const PooledSource *pooled) {
    BnFinalizeBwdArgs F = make_finalize_bwd(V, count, training, bn, cst, g);
    if (pooled) F.p_dout = pooled->dout, F.p_zsel = pooled->zsel, F.p_scale = pooled->scale, F.p_shift = pooled->shift, F.p_G = pooled->G;
    const DzJob J = make_dz_job(dz, bn.C);
    const int C = bn.C, nfin = cdiv(C, FIN_COLS), ndz = dz_job_blocks(J, C);
    ProfScope ps(st, "bn_finalize_bwd_kernel C=%d%s%s", C, ndz ? " +dZ" : "", pooled ? " +pool" : "");
    hipLaunchKernelGGL(bn_finalize_bwd_kernel, dim3(nfin + ndz), dim3(256), 0, st, F, nfin, J);
    PNPP_CHECK_LAUNCH("bn_finalize_bwd");
    return PNPP_OK;
}

int launch_post_gemm(const StatsView &V, double count, int training, const BnLayer &bn, float *cst, const BnGrads &g, const SlabReduceArgs &R,
                     hipStream_t st, const DzSide &dz) {
    const BnFinalizeBwdArgs F = make_finalize_bwd(V, count, training, bn, cst, g);
    const int C = bn.C, nsplit = R.nsplit;
    const DzJob J = make_dz_job(dz, C);
    const int total = R.Nc * R.Kvalid, nfin = cdiv(C, FIN_COLS), ndz = dz_job_blocks(J, C), nf = nfin + ndz;
    ProfScope ps(st, "post_gemm_kernel C=%d%s | N=%d K=%d split=%d", C, ndz ? " +dZ" : "", R.Nc, R.Kvalid, nsplit);
    if (nsplit == 0) {   // the weight gradient was written in place by its GEMM (one row range): nothing to reduce
        hipLaunchKernelGGL(post_gemm_kernel<64>, dim3(nf), dim3(256), 0, st, F, nfin, R, ndz, J);
    } else if (slab_reduce_vec4(R)) {
        const int groups = total / 4, epb = slab_reduce_epb4(nsplit);
        if (epb == 64) hipLaunchKernelGGL((post_gemm_kernel<64, true>), dim3(nf + cdiv(groups, 64)), dim3(256), 0, st, F, nfin, R, ndz, J);
        else if (epb == 16) hipLaunchKernelGGL((post_gemm_kernel<16, true>), dim3(nf + cdiv(groups, 16)), dim3(256), 0, st, F, nfin, R, ndz, J);
        else hipLaunchKernelGGL((post_gemm_kernel<4, true>), dim3(nf + cdiv(groups, 4)), dim3(256), 0, st, F, nfin, R, ndz, J);
    } else if (slab_reduce_wide(total, nsplit))
        hipLaunchKernelGGL(post_gemm_kernel<64>, dim3(nf + cdiv(total, 64)), dim3(256), 0, st, F, nfin, R, ndz, J);
    else
        hipLaunchKernelGGL(post_gemm_kernel<16>, dim3(nf + cdiv(total, 16)), dim3(256), 0, st, F, nfin, R, ndz, J);
    PNPP_CHECK_LAUNCH("post_gemm");
    return PNPP_OK;
}

// ---------------------------------------------------------------------------------------------
// max over the nsample axis with BatchNorm apply + ReLU folded in (pointnet_pp_8dir.py:41-42)
// first maximum wins ties (what torch.max does on the CPU)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pool_fwd_kernel(const float *__restrict__ z, const float *__restrict__ scale,
                                                       const float *__restrict__ shift, int G, int K, int C,
                                                       float *__restrict__ out, int32_t *__restrict__ arg,
                                                       float *__restrict__ origin_a, float *__restrict__ origin_b, int norigin,
                                                       float *__restrict__ zsel) {
    if (blockIdx.x == 0)  // group_all levels: the centre of every cloud is the origin (pointnet_pp_8dir.py:24); no launch of its own
        for (int i = threadIdx.x; i < norigin; i += 256) {
            if (origin_a) origin_a[i] = 0.f;
            if (origin_b) origin_b[i] = 0.f;
        }
    const size_t total = (size_t)G * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t g = i / C;
        const int c = (int)(i - g * C);
        const float sc = scale[c], sh = shift[c];
        const float *p = z + g * K * C + c;
        float best = -INFINITY, zb = 0.f;
        int bi = 0;
        int k = 0;
        for (; k + 8 <= K; k += 8) {  // eight independent strided loads in flight per lane
            float z[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) z[u] = p[(size_t)(k + u) * C];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float v = fmaxf(fmaf(z[u], sc, sh), 0.f);
                if (v > best) best = v, bi = k + u, zb = z[u];
            }
        }
        for (; k < K; ++k) {
            const float zk = p[(size_t)k * C];
            const float v = fmaxf(fmaf(zk, sc, sh), 0.f);
            if (v > best) best = v, bi = k, zb = zk;
        }
        out[i] = best;
        arg[i] = bi;
        if (zsel) zsel[i] = zb;   // the pre-BN value the maximum came from: backward reads it instead of gathering z
    }
}

// The same reduction for a level that pools over whole clouds (group_all on raw points: K = N in the thousands, few
// groups): K is cut into gridDim.z chunks, a workgroup = 64 channels x 4 interleaved row lanes reduces one chunk to a
// (value, position) partial, and pool_fwd_merge_kernel takes the first maximum over the chunks in ascending order.
__global__ void __launch_bounds__(256) pool_fwd_split_kernel(const float *__restrict__ z, const float *__restrict__ scale,
                                                             const float *__restrict__ shift, int K, int C, int chunk,
                                                             float *__restrict__ pmax, int32_t *__restrict__ parg) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int g = blockIdx.y, s = blockIdx.z;
    const int k0 = s * chunk, k1 = k0 + chunk < K ? k0 + chunk : K;
    float best = -INFINITY;
    int bi = k0;
    if (c < C) {
        const float sc = scale[c], sh = shift[c];
        const float *p = z + (size_t)g * K * C + c;
        int k = k0 + rl;
        for (; k + 12 < k1; k += 16) {  // four independent strided loads in flight per lane
            float t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = p[(size_t)(k + 4 * u) * C];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float v = fmaxf(fmaf(t[u], sc, sh), 0.f);
                if (v > best) best = v, bi = k + 4 * u;
            }
        }
        for (; k < k1; k += 4) {
            const float v = fmaxf(fmaf(p[(size_t)k * C], sc, sh), 0.f);
            if (v > best) best = v, bi = k;
        }
    }
    sv[rl][cl] = best;
    si[rl][cl] = bi;
    __syncthreads();
    if (rl == 0 && c < C) {
#pragma unroll
        for (int r = 1; r < 4; ++r) {
            const float v = sv[r][cl];
            const int i = si[r][cl];
            if (v > best || (v == best && i < bi)) best = v, bi = i;
        }
        const size_t o = ((size_t)g * gridDim.z + s) * C + c;
        pmax[o] = best;
        parg[o] = bi;
    }
}

__global__ void __launch_bounds__(256) pool_fwd_merge_kernel(const float *__restrict__ pmax, const int32_t *__restrict__ parg, int G,
                                                             int nsplit, int C, float *__restrict__ out, int32_t *__restrict__ arg,
                                                             float *__restrict__ origin_a, float *__restrict__ origin_b, int norigin) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < norigin; i += 256) {
            if (origin_a) origin_a[i] = 0.f;
            if (origin_b) origin_b[i] = 0.f;
        }
    const size_t total = (size_t)G * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t g = i / C;
        const int c = (int)(i - g * C);
        float best = -INFINITY;
        int bi = 0;
        for (int s = 0; s < nsplit; ++s) {
            const size_t o = (g * nsplit + s) * C + c;
            const float v = pmax[o];
            if (v > best) best = v, bi = parg[o];
        }
        out[i] = best;
        arg[i] = bi;
    }
}

int pool_fwd_splits(int G, int K, int C) {
    if (K < 512) return 1;  // neighbourhood-sized groups: one thread per (group, channel)
    const long long blocks = (long long)cdiv(C, 64) * G;
    int nsplit = (int)cdiv(2048, blocks);          // >= 2048 workgroups over the chip ...
    const int most = K / 64;                        // ... of at least 64 rows each
    nsplit = nsplit > most ? most : nsplit;
    return nsplit < 1 ? 1 : nsplit;
}

int launch_pool_fwd(const float *z, const float *scale, const float *shift, int G, int K, int C, float *out, int32_t *arg,
                    hipStream_t st, float *origin_a, float *origin_b, int norigin, void *part, float *zsel) {
    const int nsplit = part ? pool_fwd_splits(G, K, C) : 1;
    if (nsplit > 1) {
        const int chunk = (cdiv(K, nsplit) + 3) & ~3;
        float *pmax = (float *)part;
        int32_t *parg = (int32_t *)(pmax + (size_t)G * nsplit * C);
        {
            ProfScope ps(st, "pool_fwd_split_kernel G=%d K=%d C=%d split=%d", G, K, C, nsplit);
            hipLaunchKernelGGL(pool_fwd_split_kernel, dim3(cdiv(C, 64), G, nsplit), dim3(256), 0, st, z, scale, shift, K, C, chunk,
                               pmax, parg);
            PNPP_CHECK_LAUNCH("pool_fwd_split");
        }
        const size_t tot = (size_t)G * C;
        ProfScope ps(st, "pool_fwd_merge_kernel G=%d C=%d split=%d", G, C, nsplit);
        hipLaunchKernelGGL(pool_fwd_merge_kernel, dim3((unsigned)cdiv(tot, 256)), dim3(256), 0, st, pmax, parg, G, nsplit, C, out, arg,
                           origin_a, origin_b, norigin);
        PNPP_CHECK_LAUNCH("pool_fwd_merge");
        return PNPP_OK;
    }
    const size_t total = (size_t)G * C;
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    ProfScope ps(st, "pool_fwd_kernel G=%d K=%d C=%d", G, K, C);
    hipLaunchKernelGGL(pool_fwd_kernel, dim3(grid), dim3(256), 0, st, z, scale, shift, G, K, C, out, arg, origin_a, origin_b, norigin,
                       zsel);
    PNPP_CHECK_LAUNCH("pool_fwd");
    return PNPP_OK;
}

// backward of max + ReLU: the dense gradient (zero except at the arg-max row when the pooled value is > 0)
// is NOT written; this kernel emits the masked pooled gradient dm (G x C) and the two BatchNorm-backward
// column sums, and the consumers rebuild dy from (dm, arg) on the fly.  block = 64 channels x 4 group lanes.
// (bx, by) of ny: the block's place in the (channel blocks, group lanes) grid
__device__ __forceinline__ void pool_bwd_block(const float *__restrict__ dout, const int32_t *__restrict__ arg, const float *__restrict__ z,
                                               const float *__restrict__ scale, const float *__restrict__ shift,
                                               const float *__restrict__ mean, const float *__restrict__ istd, int G, int K, int C,
                                               float *__restrict__ dm, double *__restrict__ slab, const float *__restrict__ zsel,
                                               int policy, unsigned bx, unsigned by, unsigned ny) {
    __shared__ double red[4][2][64];
    const int cl = threadIdx.x & 63, gl = threadIdx.x >> 6;
    const int c = bx * 64 + cl;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        const float mu = mean[c], is = istd[c], sc = scale[c], sh = shift[c];
        for (int g = by * 4 + gl; g < G; g += ny * 4) {
            const size_t gi = (size_t)g * C + c;
            // the pre-BN value behind the pooled output: kept by the forward pass (zsel, a coalesced stream), or gathered --
            // one 4-byte element per (group, channel) out of a row of Z, a 64-byte line each
            const float za = zsel ? zsel[gi] : z[((size_t)g * K + arg[gi]) * C + c];
            const float d = fmaf(za, sc, sh) > 0.f ? dout[gi] : 0.f;  // ReLU'(pooled value), same expression as forward
            dm[gi] = d;
            s1 += (double)d;
            s2 += (double)d * (double)((za - mu) * is);
        }
    }
    red[gl][0][cl] = s1;
    red[gl][1][cl] = s2;
    __syncthreads();
    if (gl == 0 && c < C) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) a += red[i][0][cl], b += red[i][1][cl];
        sp_store(slab + ((size_t)by * 2 + 0) * C + c, a, (policy & ST_STAT_SLABS) != 0);
        sp_store(slab + ((size_t)by * 2 + 1) * C + c, b, (policy & ST_STAT_SLABS) != 0);
    }
}

__global__ void __launch_bounds__(256)
pool_bwd_kernel(const float *__restrict__ dout, const int32_t *__restrict__ arg, const float *__restrict__ z,
                const float *__restrict__ scale, const float *__restrict__ shift, const float *__restrict__ mean,
                const float *__restrict__ istd, int G, int K, int C, float *__restrict__ dm, double *__restrict__ slab,
                const float *__restrict__ zsel, int policy) {
    pool_bwd_block(dout, arg, z, scale, shift, mean, istd, G, K, C, dm, slab, zsel, policy, blockIdx.x, blockIdx.y, gridDim.y);
}

// The pooling backward of a level with the trailing weight-gradient reduction of the level above in the same grid: the reduction is
// read by nobody before the optimiser, the pooling launch does not read it, and as two launches each paid the launch floor alone.
// Blocks [0, nx * ny) are the pooling blocks in the order of the (nx, ny) grid -- they feed the next launch and start first; the
// rest run the reduction exactly as its own launch would (same blocks, same order of sums, same stores).  PAIR: the <16, 64> form
// of slab_reduce2_kernel, else one slab_reduce_kernel<64>.
struct PoolBwdArgs {
    const float *dout;
    const int32_t *arg;
    const float *z, *scale, *shift, *mean, *istd;
    int G, K, C;
    float *dm;
    double *slab;
    const float *zsel;
    int policy;
};
template <bool PAIR>
__global__ void __launch_bounds__(256) pool_bwd_ride_kernel(PoolBwdArgs P, int nx, int ny, SlabReduceArgs R1, int n1, SlabReduceArgs R2) {
    const int bid = blockIdx.x, npool = nx * ny;
    if (bid < npool) {
        pool_bwd_block(P.dout, P.arg, P.z, P.scale, P.shift, P.mean, P.istd, P.G, P.K, P.C, P.dm, P.slab, P.zsel, P.policy, bid % nx, bid / nx, ny);
    } else if constexpr (PAIR) {
        if (bid - npool < n1) slab_reduce_block<16>(R1, bid - npool);
        else slab_reduce_block<64>(R2, bid - npool - n1);
    } else {
        slab_reduce_block<64>(R1, bid - npool);
    }
}

int launch_pool_bwd(const float *dout, const int32_t *arg, const float *z, const float *scale, const float *shift,
                    const float *mean, const float *istd, int G, int K, int C, float *dm, double *slab, int *nslab,
                    hipStream_t st, const float *zsel, const SaTail *ride) {
    int gy = cdiv(G, 16);  // four groups per lane-row and pass
    if (gy > kMaxStatBlocks) gy = kMaxStatBlocks;
    if (gy < 1) gy = 1;
    *nslab = gy;
    if (ride && ride->kind != PNPP_SA_TAIL_NONE) {
        if (!slab_tail_rides(*ride)) PNPP_TRY(launch_slab_tail(*ride, st));   // no merged kernel for this form: its own launch, first
        else {
            const SlabReduceArgs &R1 = ride->R1, &R2 = ride->R2;
            const PoolBwdArgs P{dout, arg, z, scale, shift, mean, istd, G, K, C, dm, slab, zsel, store_policy()};
            const int nx = cdiv(C, 64), nride = slab_tail_blocks(*ride);
            if (ride->kind == PNPP_SA_TAIL_SLAB_REDUCE2) {
                bool w1, w2;
                int n1, n2;
                slab_reduce2_plan(R1, R2, &w1, &w2, &n1, &n2);
                ProfScope ps(st, "pool_bwd_kernel G=%d K=%d C=%d + slab_reduce2 N=%d K=%d split=%d | N=%d K=%d split=%d", G, K, C, R1.Nc,
                             R1.Kvalid, R1.nsplit, R2.Nc, R2.Kvalid, R2.nsplit);
                hipLaunchKernelGGL(pool_bwd_ride_kernel<true>, dim3(nx * gy + nride), dim3(256), 0, st, P, nx, gy, R1, n1, R2);
            } else {
                ProfScope ps(st, "pool_bwd_kernel G=%d K=%d C=%d + slab_reduce N=%d K=%d split=%d", G, K, C, R1.Nc, R1.Kvalid, R1.nsplit);
                hipLaunchKernelGGL(pool_bwd_ride_kernel<false>, dim3(nx * gy + nride), dim3(256), 0, st, P, nx, gy, R1, 0, R1);
            }
            PNPP_CHECK_LAUNCH("pool_bwd(+tail)");
            return PNPP_OK;
        }
    }
    ProfScope ps(st, "pool_bwd_kernel G=%d K=%d C=%d", G, K, C);
    hipLaunchKernelGGL(pool_bwd_kernel, dim3(cdiv(C, 64), gy), dim3(256), 0, st, dout, arg, z, scale, shift, mean, istd, G, K, C,
                       dm, slab, zsel, store_policy());
    PNPP_CHECK_LAUNCH("pool_bwd");
    return PNPP_OK;
}

int launch_fill_zero(void *p, size_t bytes, hipStream_t st) {
    if (bytes == 0) return PNPP_OK;
    hipError_t e = hipMemsetAsync(p, 0, bytes, st);
    if (e != hipSuccess) {
        set_error("memset failed: %s", hipGetErrorString(e));
        return PNPP_ERR_LAUNCH;
    }
    return PNPP_OK;
}

}  // namespace pnpp
