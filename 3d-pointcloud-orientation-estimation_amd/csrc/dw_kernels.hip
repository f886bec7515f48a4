// dw_kernels.hip -- the weight-gradient products of the set-abstraction layers: dW = dZ^T A2 from global memory (dw_kernel), through
// LDS for the small-M levels (dw_lds), for an xyz-only layer 0 (dw_xyz); layer 0 convolved before the gather and its backward scatter
// (gather_rel_stats, scatter_dz); and the launch that pairs dA with dW on a small-M level (da_dw).  The operands are built by the
// loaders of operand_load.h; partial products go to slabs that bn_pool_kernels.hip reduces.
#include "gemm_smallm.h"
#include "launch.h"
#include "split_prims.h"

namespace pnpp {

// ---------------------------------------------------------------------------------------------
// dW = dZ^T * A2 : both operands are read straight from global memory in MFMA layout -- the lane
// index is the channel, which is the contiguous dimension of every row-major activation, so each
// half-wave load is one 128-byte segment.  Reduction runs over rows; each wave owns one
// (32*CT x 32*KT) output tile and one row range, partial tiles go to a slab (deterministic).
// ---------------------------------------------------------------------------------------------
template <int DZMODE, int A2MODE, int CT, int KT>
__global__ void __launch_bounds__(256)
dw_kernel(const AOperand dz, const AOperand a2, int M, int Nc, int Kp, int tilesC, int tilesK, int rows_per_split,
          int kp_pad, float *__restrict__ slab, int policy) {
    constexpr int U = 4;  // row pairs fetched per batch: U*(CT+KT) independent loads in flight per lane
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int tiles = tilesC * tilesK;
    const int tile = gw % tiles, split = gw / tiles;
    const int r0 = min(M, split * rows_per_split);  // an empty range still writes its (zero) slab tile
    const int r1 = min(M, r0 + rows_per_split);
    const int c0 = (tile % tilesC) * 32 * CT, k0 = (tile / tilesC) * 32 * KT;

    ChanConst cc[CT], ck[KT];
#pragma unroll
    for (int i = 0; i < CT; ++i) cc[i] = load_chan_const<DZMODE>(dz, c0 + i * 32 + l31, Nc);
#pragma unroll
    for (int j = 0; j < KT; ++j) ck[j] = load_chan_const<A2MODE>(a2, k0 + j * 32 + l31, Kp);

    f32x16 acc[CT][KT];
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int j = 0; j < KT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // A_DZ_POOL: a batch of 2U rows lies inside one group when K % 2U == 0 (row ranges start on multiples of 2U),
    // so the pooled gradient / arg-max of the group are fetched once per batch instead of once per row
    const bool grp_batch = (DZMODE == A_DZ_POOL) && (dz.K % (2 * U) == 0) && (r0 % (2 * U) == 0);
    for (int row = r0; row < r1; row += 2 * U) {
        float2 fa[U][CT], fb[U][KT];
        float gdm[CT];
        int garg[CT], gk0 = 0;
        if (DZMODE == A_DZ_POOL && grp_batch) {
            const int g = row / dz.K;
            gk0 = row - g * dz.K;
#pragma unroll
            for (int i = 0; i < CT; ++i) {
                const int c = min(c0 + i * 32 + l31, Nc - 1);
                gdm[i] = dz.a[(size_t)g * dz.lda + c];
                garg[i] = dz.arg[(size_t)g * dz.lda + c];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = row + 2 * u + lh;
#pragma unroll
            for (int i = 0; i < CT; ++i) {
                if (DZMODE == A_DZ_POOL && grp_batch) {
                    const int c = min(c0 + i * 32 + l31, Nc - 1);
                    fa[u][i].x = (gk0 + 2 * u + lh == garg[i]) ? gdm[i] : 0.f;
                    fa[u][i].y = dz.z[(size_t)min(m, M - 1) * dz.lda + c];
                } else {
                    fa[u][i] = fetch_a1<DZMODE>(dz, m, c0 + i * 32 + l31, Nc, M);
                }
            }
#pragma unroll
            for (int j = 0; j < KT; ++j) fb[u][j] = fetch_a1<A2MODE>(a2, m, k0 + j * 32 + l31, Kp, M);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = row + 2 * u + lh < r1;
            float a[CT], b[KT];
#pragma unroll
            for (int i = 0; i < CT; ++i) a[i] = xform_a1<DZMODE>(fa[u][i], cc[i], c0 + i * 32 + l31, Nc, ok);
#pragma unroll
            for (int j = 0; j < KT; ++j) b[j] = xform_a1<A2MODE>(fb[u][j], ck[j], k0 + j * 32 + l31, Kp, ok);
#pragma unroll
            for (int i = 0; i < CT; ++i)
#pragma unroll
                for (int j = 0; j < KT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    float *o = slab + (size_t)split * Nc * kp_pad;
    sp_with_policy((policy & ST_DW_SLABS) != 0, [&](auto wt) {
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
            for (int j = 0; j < KT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = c0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const int k = k0 + j * 32 + l31;
                    if (c < Nc && k < kp_pad) sp_store(o + (size_t)c * kp_pad + k, acc[i][j][r], wt());
                }
    });
}

// ---------------------------------------------------------------------------------------------
// dW of an xyz-only layer 0 (SA1: C x 3): dW[c][k] = sum_m dZ[m][c] * (xyz[nbr(m)][k] - centre(m)[k]).
// The 64 x 64 MFMA tiles of dw_kernel would spend 61 of their 64 reduction columns on padding; this is a streaming
// VALU kernel instead: a workgroup takes 256 consecutive rows, stages their three relative coordinates in LDS (one
// row per thread: neighbour index, gather, float32 subtraction as in the forward) and then walks the rows with
// lane = channel (64 channels x 4 row lanes), so dY and Z are read once, fully coalesced, and dZ is rebuilt on the
// fly.  Output: one partial [C][4] per workgroup in the slab layout slab_reduce expects (pitch 4).
// ---------------------------------------------------------------------------------------------
template <int DZMODE, int A2MODE>  // A2MODE: A_GATHER (neighbourhoods) or A_CONCAT (group_all on raw coordinates: centre = origin)
__global__ void __launch_bounds__(256)
dw_xyz_kernel(const AOperand dz, const AOperand a2, int M, int C, float *__restrict__ slab, int policy) {
    __shared__ float rel[256][4];
    __shared__ float red[4][64][3];
    const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6;
    const int m0 = blockIdx.x * 256;
    {  // this thread's row: relative coordinates, zero for rows beyond M
        const float2 x = fetch_a1<A2MODE>(a2, m0 + tid, 0, 3, M);
        const float2 y = fetch_a1<A2MODE>(a2, m0 + tid, 1, 3, M);
        const float2 z = fetch_a1<A2MODE>(a2, m0 + tid, 2, 3, M);
        const float okf = (m0 + tid < M) ? 1.f : 0.f;
        rel[tid][0] = __fsub_rn(x.x, x.y) * okf;
        rel[tid][1] = __fsub_rn(y.x, y.y) * okf;
        rel[tid][2] = __fsub_rn(z.x, z.y) * okf;
        rel[tid][3] = 0.f;
    }
    __syncthreads();
    for (int c0 = blockIdx.y * 64; c0 < C; c0 += gridDim.y * 64) {
        const int c = c0 + cl;
        const ChanConst cc = load_chan_const<DZMODE>(dz, min(c, C - 1), C);
        float a0 = 0.f, a1 = 0.f, a2s = 0.f;
#pragma unroll 8
        for (int r = rl; r < 256; r += 4) {
            const float2 f = fetch_a1<DZMODE>(dz, m0 + r, c, C, M);
            const float g = xform_a1<DZMODE>(f, cc, c, C, true);  // rows >= M meet zero coordinates
            const float4 q = *reinterpret_cast<const float4 *>(rel[r]);
            a0 = fmaf(g, q.x, a0), a1 = fmaf(g, q.y, a1), a2s = fmaf(g, q.z, a2s);
        }
        red[rl][cl][0] = a0, red[rl][cl][1] = a1, red[rl][cl][2] = a2s;
        __syncthreads();
        if (tid < 192) {
            const int ch = tid / 3, k = tid - 3 * ch;
            if (c0 + ch < C)
                sp_store(slab + ((size_t)blockIdx.x * C + c0 + ch) * 4 + k, (red[0][ch][k] + red[1][ch][k]) + (red[2][ch][k] + red[3][ch][k]),
                         (policy & ST_DW_SLABS) != 0);
        }
        __syncthreads();
    }
}

// number of partial slabs launch_dw_xyz writes (pitch 4), for sizing
int dw_xyz_splits(int M) { return cdiv(M, 256); }

template <int A2MODE>
static int launch_dw_xyz_a2(const AOperand &dz, int C, const AOperand &a2, int M, float *slab, dim3 grid, hipStream_t st) {
    switch (dz.mode) {
        case A_PLAIN: hipLaunchKernelGGL((dw_xyz_kernel<A_PLAIN, A2MODE>), grid, dim3(256), 0, st, dz, a2, M, C, slab, store_policy()); break;
        case A_DZ: hipLaunchKernelGGL((dw_xyz_kernel<A_DZ, A2MODE>), grid, dim3(256), 0, st, dz, a2, M, C, slab, store_policy()); break;
        case A_DZ_POOL: hipLaunchKernelGGL((dw_xyz_kernel<A_DZ_POOL, A2MODE>), grid, dim3(256), 0, st, dz, a2, M, C, slab, store_policy()); break;
        default: set_error("dw_xyz: bad dZ mode %d", dz.mode); return PNPP_ERR_ARG;
    }
    return PNPP_OK;
}

int launch_dw_xyz(const AOperand &dz, int C, const AOperand &a2, int M, float *slab, hipStream_t st) {
    PNPP_REQUIRE((a2.mode == A_GATHER || a2.mode == A_CONCAT) && a2.D == 0, PNPP_ERR_ARG,
                 "dw_xyz: the second operand must be xyz-only (gathered or whole-cloud)");
    PNPP_REQUIRE(M > 0 && C > 0, PNPP_ERR_ARG, "dw_xyz: non-positive size");
    const dim3 grid(dw_xyz_splits(M), 1);
    ProfScope ps(st, "dw_xyz_kernel<A%d,A%d> M=%d N=%d K=3 grid=%dx1", dz.mode, a2.mode, M, C, grid.x);
    const int rc = a2.mode == A_GATHER ? launch_dw_xyz_a2<A_GATHER>(dz, C, a2, M, slab, grid, st)
                                       : launch_dw_xyz_a2<A_CONCAT>(dz, C, a2, M, slab, grid, st);
    if (rc != PNPP_OK) return rc;
    PNPP_CHECK_LAUNCH("dw_xyz");
    return PNPP_OK;
}

// ---------------------------------------------------------------------------------------------
// Layer 0 of a grouped set abstraction with input features ("convolve, then gather").  The 1x1 convolution is linear,
// so for row (group s, neighbour k) with source point j = idx[s][k]
//     z = W_xyz (x_j - c_s) + W_f f_j  =  P[j] + W_xyz (x_j - c_s),      P = F W_f^T   (one row per SOURCE point)
// P costs B*N rows of GEMM instead of B*S*K (8x fewer for SA2); the relative-coordinate term keeps the reference's
// float32 subtraction (pointnet_pp_8dir.py:28-31) and is three FMAs per output.  This kernel builds Z (row-major,
// pre-BN, no bias: BatchNorm cancels it) and the per-channel sum / sum of squares partials of the BN statistics.
// Thread = 4 channels of one row; a workgroup walks `rpb` consecutive rows, 256 / (C/4) at a time.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
gather_rel_stats_kernel(const float *__restrict__ P, const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                        const int32_t *__restrict__ idx, const float *__restrict__ W0, int ldw, int N, int S, int K, int M,
                        int C, int rpb, float *__restrict__ z, double *__restrict__ slab, int policy) {
    extern __shared__ __attribute__((aligned(16))) double gred[];  // [RPP][2][C]
    const int LPR = C >> 2, RPP = 256 / LPR;
    const int cl = threadIdx.x % LPR, rl = threadIdx.x / LPR, c4 = cl * 4;
    float wx[4], wy[4], wz[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float *w = W0 + (size_t)(c4 + e) * ldw;
        wx[e] = w[0], wy[e] = w[1], wz[e] = w[2];
    }
    const int r0 = blockIdx.x * rpb, r1 = min(M, r0 + rpb);
    double d1[4] = {0.0, 0.0, 0.0, 0.0}, d2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int rb = r0 + rl; rb < r1; rb += 4 * RPP) {
        float4 p[4];
        float rx[4], ry[4], rz[4], ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // four rows in flight per thread
            const int r = rb + u * RPP;
            const int rc = min(r, r1 - 1);
            ok[u] = r < r1 ? 1.f : 0.f;
            const int grp = rc / K;
            const size_t src = (size_t)(grp / S) * N + idx[rc];
            p[u] = *reinterpret_cast<const float4 *>(P + src * C + c4);
            const float *x = xyz + src * 3, *c = new_xyz + (size_t)grp * 3;
            rx[u] = __fsub_rn(x[0], c[0]), ry[u] = __fsub_rn(x[1], c[1]), rz[u] = __fsub_rn(x[2], c[2]);
        }
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v[4] = {p[u].x, p[u].y, p[u].z, p[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = fmaf(rz[u], wz[e], fmaf(ry[u], wy[e], fmaf(rx[u], wx[e], v[e])));
                const float m = v[e] * ok[u];
                s1[e] += m, s2[e] = fmaf(m, m, s2[e]);
            }
            const int r = rb + u * RPP;
            // (plain under every policy: 16-byte write-through buffer stores did not make this launch shorter)
            if (r < r1) *reinterpret_cast<float4 *>(z + (size_t)r * C + c4) = make_float4(v[0], v[1], v[2], v[3]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) d1[e] += (double)s1[e], d2[e] += (double)s2[e];
    }
    if (slab == nullptr) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        gred[(rl * 2 + 0) * C + c4 + e] = d1[e];
        gred[(rl * 2 + 1) * C + c4 + e] = d2[e];
    }
    __syncthreads();
    for (int f = threadIdx.x; f < 2 * C; f += 256) {
        const int which = f / C, c = f - which * C;
        double t = 0.0;
        for (int w = 0; w < RPP; ++w) t += gred[(w * 2 + which) * C + c];
        sp_store(slab + ((size_t)blockIdx.x * 2 + which) * C + c, t, (policy & ST_STAT_SLABS) != 0);
    }
}

bool delayed_layer0_ok(int C) {  // C/4 lanes per row must divide the 256-thread workgroup; the scatter holds C <= 512
    return C >= 32 && C <= 512 && (C & (C - 1)) == 0;
}

int launch_gather_rel_stats(const float *P, const AOperand &geo, const float *W0, int ldw, int M, int C, float *z,
                            double *slab, int *nslab, hipStream_t st) {
    PNPP_REQUIRE(delayed_layer0_ok(C) && geo.mode == A_GATHER, PNPP_ERR_ARG, "gather_rel_stats: unsupported width %d", C);
    const int rpp = 256 / (C / 4);
    int rpb = 64;  // rows per workgroup: a multiple of the 4 * rpp rows in flight, at most kMaxStatBlocks workgroups
    while (rpb < 4 * rpp || cdiv(M, rpb) > kMaxStatBlocks) rpb *= 2;
    const int grid = cdiv(M, rpb);
    if (nslab) *nslab = grid;
    ProfScope ps(st, "gather_rel_stats_kernel M=%d C=%d grid=%d", M, C, grid);
    hipLaunchKernelGGL(gather_rel_stats_kernel, dim3(grid), dim3(256), (size_t)rpp * 2 * C * sizeof(double), st, P, geo.xyz,
                       geo.new_xyz, geo.idx, W0, ldw, geo.N, geo.S, geo.K, M, C, rpb, z, slab, store_policy());
    PNPP_CHECK_LAUNCH("gather_rel_stats");
    return PNPP_OK;
}

// ---------------------------------------------------------------------------------------------
// Backward of the same layer: the gradient reaches the feature weights and the source features only through
//     G[j] = sum over the rows r of the cloud with idx[r] == j of dZ[r]            (one row per SOURCE point)
// (dW_f = G^T F and dF = G W_f are then B*N-row GEMMs).  One wavefront per source point scans its cloud's neighbour
// lists in order, 1024 entries per pass, compacts the matching rows into a list (ballot + prefix count, so list order
// is row order) and adds them in that order: a fixed summation order, no atomics.  dZ is rebuilt on the fly from the
// masked upstream gradient and Z (A_DZ): two coalesced row reads per match, up to eight matches in flight.  Lane = 2 channels of each 128-channel chunk.  The same pass accumulates the C x 3 gradient of
// the coordinate columns, dW_xyz = sum_r dZ[r] (x_j - c_s)^T, as one [C][4] partial per workgroup (slab_reduce layout).
// ---------------------------------------------------------------------------------------------
constexpr int SCW = 8;       // wavefronts (= source points) per workgroup
constexpr int SCWIN = 1024;  // neighbour-list entries examined per pass
template <int NCH>
__global__ void __launch_bounds__(SCW * 64)
scatter_dz_kernel(const AOperand dz, const AOperand geo, int Mc, int C, int total, float *__restrict__ G,
                  float *__restrict__ wslab) {
    constexpr int UB = NCH == 1 ? 8 : 4;  // matching rows fetched per batch
    __shared__ int hl[SCW][SCWIN];
    __shared__ float wred[SCW][NCH * 128][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int N = geo.N;
    const int dst = min(blockIdx.x * SCW + wv, total - 1);  // b * N + n; a surplus wave repeats the last point, writes nothing
    const bool live = blockIdx.x * SCW + wv < total;
    const int b = dst / N, n = dst - b * N;
    const int32_t *ib = geo.idx + (size_t)b * Mc;
    const size_t row0 = (size_t)b * Mc;
    const float px = geo.xyz[(size_t)dst * 3], py = geo.xyz[(size_t)dst * 3 + 1], pz = geo.xyz[(size_t)dst * 3 + 2];
    const float *cb = geo.new_xyz + (size_t)b * geo.S * 3;
    float2 cg[NCH], cmu[NCH], cis[NCH], c1[NCH], c2[NCH], acc[NCH], ax[NCH], ay[NCH], az[NCH];
    int cc[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        cc[j] = min(j * 128 + 2 * lane, C - 2);
        cg[j] = make_float2(1.f, 1.f);
        cmu[j] = cis[j] = c1[j] = c2[j] = acc[j] = ax[j] = ay[j] = az[j] = make_float2(0.f, 0.f);
        if (dz.mode == A_DZ) {
            const float *p = dz.cst + cc[j];
            cg[j] = *reinterpret_cast<const float2 *>(p), cmu[j] = *reinterpret_cast<const float2 *>(p + dz.C);
            cis[j] = *reinterpret_cast<const float2 *>(p + 2 * dz.C), c1[j] = *reinterpret_cast<const float2 *>(p + 3 * dz.C);
            c2[j] = *reinterpret_cast<const float2 *>(p + 4 * dz.C);
        }
    }
    const float *zsrc = dz.mode == A_DZ ? dz.z : dz.a;  // a materialised dZ (small levels) passes through: g = 1, c1 = c2 = 0
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int w0 = 0; w0 < Mc; w0 += SCWIN) {  // uniform over the workgroup
        // 1. the rows of this window that point at n, in row order, as a list in LDS
        int v[SCWIN / 64];
#pragma unroll
        for (int q = 0; q < SCWIN / 64; ++q) v[q] = ib[min(w0 + q * 64 + lane, Mc - 1)];
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < SCWIN / 64; ++q) {
            const int m = w0 + q * 64 + lane;
            const bool mine = live && m < Mc && v[q] == n;
            const unsigned long long bal = __ballot(mine);
            if (mine) hl[wv][cnt + __popcll(bal & below)] = m;
            cnt += __popcll(bal);
        }
        __syncthreads();
        // 2. their dZ rows, UB at a time, added in list order
        for (int i = 0; i < cnt; i += UB) {  // cnt is wave-uniform
            int pos[UB];
            float mk[UB], rx[UB], ry[UB], rz[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                mk[u] = i + u < cnt ? 1.f : 0.f;
                pos[u] = hl[wv][min(i + u, cnt - 1)];
                const float *c = cb + (size_t)(pos[u] / geo.K) * 3;  // the forward's float32 subtraction
                rx[u] = __fsub_rn(px, c[0]) * mk[u], ry[u] = __fsub_rn(py, c[1]) * mk[u], rz[u] = __fsub_rn(pz, c[2]) * mk[u];
            }
            float2 gy[UB][NCH], gz[UB][NCH];
#pragma unroll
            for (int u = 0; u < UB; ++u)
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    const size_t o = (row0 + pos[u]) * dz.lda + cc[j];
                    gy[u][j] = *reinterpret_cast<const float2 *>(dz.a + o);
                    gz[u][j] = *reinterpret_cast<const float2 *>(zsrc + o);
                }
#pragma unroll
            for (int u = 0; u < UB; ++u)
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    const float vx = cg[j].x * (gy[u][j].x - c1[j].x - (gz[u][j].x - cmu[j].x) * cis[j].x * c2[j].x);
                    const float vy = cg[j].y * (gy[u][j].y - c1[j].y - (gz[u][j].y - cmu[j].y) * cis[j].y * c2[j].y);
                    acc[j].x = fmaf(vx, mk[u], acc[j].x), acc[j].y = fmaf(vy, mk[u], acc[j].y);
                    ax[j].x = fmaf(vx, rx[u], ax[j].x), ax[j].y = fmaf(vy, rx[u], ax[j].y);
                    ay[j].x = fmaf(vx, ry[u], ay[j].x), ay[j].y = fmaf(vy, ry[u], ay[j].y);
                    az[j].x = fmaf(vx, rz[u], az[j].x), az[j].y = fmaf(vy, rz[u], az[j].y);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = j * 128 + 2 * lane;
        if (live && c < C) *reinterpret_cast<float2 *>(G + (size_t)dst * C + c) = acc[j];
        wred[wv][c][0] = ax[j].x, wred[wv][c][1] = ay[j].x, wred[wv][c][2] = az[j].x;
        wred[wv][c + 1][0] = ax[j].y, wred[wv][c + 1][1] = ay[j].y, wred[wv][c + 1][2] = az[j].y;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < C * 3; f += SCW * 64) {  // this workgroup's share of dW_xyz: [C][4] partial, waves in order
        const int c = f / 3, k = f - 3 * c;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < SCW; ++w) t += wred[w][c][k];
        wslab[((size_t)blockIdx.x * C + c) * 4 + k] = t;
    }
}

int scatter_dz_splits(int rows) { return cdiv(rows, SCW); }

int launch_scatter_dz(const AOperand &dz, const AOperand &geo, int B, int Mc, int C, float *G, float *wslab, hipStream_t st) {
    PNPP_REQUIRE((dz.mode == A_PLAIN || (dz.mode == A_DZ && dz.C == C)) && dz.lda == C && delayed_layer0_ok(C), PNPP_ERR_ARG,
                 "scatter_dz: bad operand");
    PNPP_REQUIRE(geo.mode == A_GATHER && geo.S * geo.K == Mc, PNPP_ERR_ARG, "scatter_dz: bad geometry");
    const int total = B * geo.N;
    ProfScope ps(st, "scatter_dz_kernel B=%d N=%d C=%d M=%d", B, geo.N, C, Mc);
    const dim3 grid(scatter_dz_splits(total));
    if (C <= 128) hipLaunchKernelGGL(scatter_dz_kernel<1>, grid, dim3(SCW * 64), 0, st, dz, geo, Mc, C, total, G, wslab);
    else if (C <= 256) hipLaunchKernelGGL(scatter_dz_kernel<2>, grid, dim3(SCW * 64), 0, st, dz, geo, Mc, C, total, G, wslab);
    else hipLaunchKernelGGL(scatter_dz_kernel<4>, grid, dim3(SCW * 64), 0, st, dz, geo, Mc, C, total, G, wslab);
    PNPP_CHECK_LAUNCH("scatter_dz");
    return PNPP_OK;
}

// ---------------------------------------------------------------------------------------------
// dW for the small-M levels (group_all: M = 32 B rows, wide layers).  dw_kernel's waves each pull their own operand
// rows from L2 one dword per lane; here a workgroup owns a 128 x 128 block of dW over one row range, stages 32-row
// chunks of both operands through LDS with 16-byte loads (8 per thread and chunk instead of 64 dword loads per lane),
// and its four waves (64 x 64 each, 2 x 2 MFMA tiles) read them back lane-per-column -- every staged element feeds two
// MFMA tiles.  Same partial-slab output as dw_kernel (slab[split][c][kp_pad]).
// ---------------------------------------------------------------------------------------------
// the 64 x 64 accumulators of a wave (2 x 2 MFMA tiles) into its partial: rows cb + 32 i + (r & 3) + 8 (r >> 2), columns kb + 32 j
template <bool WT>
__device__ __forceinline__ void dw_lds_tail(float *__restrict__ o, const f32x16 (&acc)[2][2], int cb, int kb, int Nc, int kp_pad) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = kb + j * 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cb + i * 32 + (r & 3) + 8 * (r >> 2);
                if (c < Nc && k < kp_pad) sp_store(o + (size_t)c * kp_pad + k, acc[i][j][r], WT);
            }
        }
}

template <int DZMODE, int A2MODE, bool POLICY>   // POLICY: the tail's stores take wt_dw (da_dw_kernel); else they are plain (dw_lds_kernel)
__device__ __forceinline__ void dw_lds_body(const AOperand &dz, const AOperand &a2, int M, int Nc, int Kp, int tilesC, int tilesK, int rps,
                                            int kp_pad, float *__restrict__ slab, int bx, const bool wt_dw) {
    __shared__ __attribute__((aligned(16))) float Dz[32][128];
    __shared__ __attribute__((aligned(16))) float A2[32][128];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int tiles = tilesC * tilesK;
    const int tile = bx % tiles, split = bx / tiles;
    const int c0 = (tile % tilesC) * 128, k0 = (tile / tilesC) * 128;
    const int r0 = min(M, split * rps), r1 = min(M, r0 + rps);  // an empty range still writes its (zero) slab block
    const int wc = wave >> 1, wk = wave & 1;
    const int q4 = 4 * (tid & 31), rb = tid >> 5;  // staging map: 4 columns of rows rb + 8 i

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    RawA nd[4], na[4];
    auto fetch = [&](int m0) {  // rows >= r1 belong to the next split: r1 plays M for the loaders (clamped loads, zeroed values)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            nd[i] = fetch_a4<DZMODE>(dz, m0 + rb + 8 * i, c0 + q4, r1, Nc);
            na[i] = fetch_a4<A2MODE>(a2, m0 + rb + 8 * i, k0 + q4, r1, Kp);
        }
    };
    if (r0 < r1) fetch(r0);
    for (int m0 = r0; m0 < r1; m0 += 32) {
        __syncthreads();  // the previous chunk's operand reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v[4];
            xform_a4<DZMODE>(dz, nd[i], m0 + rb + 8 * i, c0 + q4, r1, Nc, v);
            *reinterpret_cast<float4 *>(&Dz[rb + 8 * i][q4]) = make_float4(v[0], v[1], v[2], v[3]);
            xform_a4<A2MODE>(a2, na[i], m0 + rb + 8 * i, k0 + q4, r1, Kp, v);
            *reinterpret_cast<float4 *>(&A2[rb + 8 * i][q4]) = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        if (m0 + 32 < r1) fetch(m0 + 32);  // the next chunk's loads fly during the MFMA loop
        const float *pd = &Dz[lh][wc * 64 + l31], *pa = &A2[lh][wk * 64 + l31];
#pragma unroll 4
        for (int rp = 0; rp < 16; ++rp) {  // reduction index = row 2 rp + lh of the chunk
            const float d0 = pd[rp * 256], d1 = pd[rp * 256 + 32], b0 = pa[rp * 256], b1 = pa[rp * 256 + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(d0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(d0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(d1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(d1, b1, acc[1][1], 0, 0, 0);
        }
    }
    float *o = slab + (size_t)split * Nc * kp_pad;
    // (a function, not a lambda: through a lambda's captures dw_lds_kernel<A0,A3> takes 66 registers instead of 60 and loses a wave per SIMD)
    if constexpr (POLICY) {
        if (wt_dw) dw_lds_tail<true>(o, acc, c0 + wc * 64 + 4 * lh, k0 + wk * 64 + l31, Nc, kp_pad);
        else dw_lds_tail<false>(o, acc, c0 + wc * 64 + 4 * lh, k0 + wk * 64 + l31, Nc, kp_pad);
    } else {
        dw_lds_tail<false>(o, acc, c0 + wc * 64 + 4 * lh, k0 + wk * 64 + l31, Nc, kp_pad);
    }
}

template <int DZMODE, int A2MODE>
__global__ void __launch_bounds__(256)
dw_lds_kernel(const AOperand dz, const AOperand a2, int M, int Nc, int Kp, int tilesC, int tilesK, int rps, int kp_pad,
              float *__restrict__ slab) {
    // (plain under every policy: the launches of this kernel are not in the measured step; da_dw_kernel, which shares the body, takes it)
    dw_lds_body<DZMODE, A2MODE, false>(dz, a2, M, Nc, Kp, tilesC, tilesK, rps, kp_pad, slab, blockIdx.x, false);
}

// The two products of a small-M backward layer that only share their input -- dA = dZ W (32 x 32 split-K tiles) and
// dW = dZ^T A (LDS-staged 128 x 128 blocks) -- in ONE launch: the first g1 workgroups take the GEMM tiles, the rest
// the dW blocks.  These launches are latency-bound, so the pair costs about as much as the longer of the two.
template <int EMODE, int A2MODE>
__global__ void __launch_bounds__(256)
da_dw_kernel(const AOperand dzA, const BOperand W, int M, int Nout, int Kd, const Epilogue E, int g1x, int g1, const AOperand a2, int Nc,
             int Kp, int tilesC, int tilesK, int rps, int kp_pad, float *__restrict__ slab) {
    if ((int)blockIdx.x < g1)
        gemm_smallm_body<A_PLAIN, EMODE, false, 4>(dzA, W, M, Nout, Kd, E, blockIdx.x % g1x, blockIdx.x / g1x, g1);
    else
        dw_lds_body<A_PLAIN, A2MODE, true>(dzA, a2, M, Nc, Kp, tilesC, tilesK, rps, kp_pad, slab, blockIdx.x - g1, (E.store_policy & ST_DW_SLABS) != 0);
}

void dw_plan(int M, int Nc, int Kp, int *nsplit, int *kp_pad) {
    const int tilesC = cdiv(Nc, 64), tilesK = cdiv(Kp, 64);
    const int tiles = tilesC * tilesK;
    // aim for ~2048 waves (2 per SIMD), at least 64 rows per wave (32 for the small-M layers, whose waves are latency
    // bound: twice the waves in flight beats the doubled slab count), at most 1024 partial slabs
    int split = cdiv(2048, tiles);
    const int max_split = cdiv(M, M <= 4096 ? 32 : 64);
    if (split > max_split) split = max_split;
    if (split > 1024) split = 1024;
    if (split < 1) split = 1;
    *nsplit = split;
    *kp_pad = tilesK * 64;
}

int launch_dw(const AOperand &dz, int Nc, const AOperand &a2, int Kp, int M, float *slab, int nsplit, int kp_pad,
              hipStream_t st) {
    PNPP_REQUIRE(M > 0 && Nc > 0 && Kp > 0 && nsplit > 0, PNPP_ERR_ARG, "dw: non-positive size");
    const int tilesC = cdiv(Nc, 64), tilesK = cdiv(Kp, 64);
    PNPP_REQUIRE(kp_pad == tilesK * 64, PNPP_ERR_ARG, "dw: kp_pad mismatch");
    int rps = cdiv(M, nsplit);
    rps = (rps + 7) & ~7;  // multiple of 8: a fetch batch (4 row pairs) never straddles two splits or two groups
    if (M <= 4096 && Nc >= 128 && Kp >= 128 && dz.mode == A_PLAIN && (dz.lda & 3) == 0 && ((uintptr_t)dz.a & 15) == 0 &&
        (a2.mode == A_PLAIN || a2.mode == A_BNRELU || a2.mode == A_CONCAT) &&
        (a2.mode == A_CONCAT || ((a2.lda & 3) == 0 && ((uintptr_t)a2.a & 15) == 0))) {
        // small-M, wide layers: LDS-staged 128 x 128 blocks
        const int tc = cdiv(Nc, 128), tk = cdiv(Kp, 128);
        const dim3 grid(tc * tk * nsplit);
        ProfScope ps(st, "dw_lds_kernel<A%d,A%d> M=%d N=%d K=%d split=%d grid=%d", dz.mode, a2.mode, M, Nc, Kp, nsplit, grid.x);
        switch (a2.mode) {
            case A_PLAIN:
                hipLaunchKernelGGL((dw_lds_kernel<A_PLAIN, A_PLAIN>), grid, dim3(256), 0, st, dz, a2, M, Nc, Kp, tc, tk, rps, kp_pad, slab);
                break;
            case A_BNRELU:
                hipLaunchKernelGGL((dw_lds_kernel<A_PLAIN, A_BNRELU>), grid, dim3(256), 0, st, dz, a2, M, Nc, Kp, tc, tk, rps, kp_pad, slab);
                break;
            default:
                hipLaunchKernelGGL((dw_lds_kernel<A_PLAIN, A_CONCAT>), grid, dim3(256), 0, st, dz, a2, M, Nc, Kp, tc, tk, rps, kp_pad, slab);
                break;
        }
        PNPP_CHECK_LAUNCH("dw(lds)");
        return PNPP_OK;
    }
    const int waves = tilesC * tilesK * nsplit;
    const dim3 grid(cdiv(waves, 4)), block(256);
    ProfScope ps(st, "dw_kernel<A%d,A%d> M=%d N=%d K=%d split=%d grid=%dx1", dz.mode, a2.mode, M, Nc, Kp, nsplit, grid.x);
#define PNPP_DW(DM, AM)                                                                                              \
    hipLaunchKernelGGL((dw_kernel<DM, AM, 2, 2>), grid, block, 0, st, dz, a2, M, Nc, Kp, tilesC, tilesK, rps, kp_pad, slab, store_policy()); \
    break;
#define PNPP_DW_BY_A(DM)                         \
    switch (a2.mode) {                           \
        case A_PLAIN: PNPP_DW(DM, A_PLAIN)       \
        case A_BNRELU: PNPP_DW(DM, A_BNRELU)     \
        case A_GATHER: PNPP_DW(DM, A_GATHER)     \
        case A_CONCAT: PNPP_DW(DM, A_CONCAT)     \
        default: set_error("dw: bad A2 mode %d", a2.mode); return PNPP_ERR_ARG; \
    }                                            \
    break;
    switch (dz.mode) {
        case A_PLAIN: PNPP_DW_BY_A(A_PLAIN)
        case A_DZ: PNPP_DW_BY_A(A_DZ)
        case A_DZ_POOL: PNPP_DW_BY_A(A_DZ_POOL)
        default: set_error("dw: bad dZ mode %d", dz.mode); return PNPP_ERR_ARG;
    }
#undef PNPP_DW_BY_A
#undef PNPP_DW
    PNPP_CHECK_LAUNCH("dw");
    return PNPP_OK;
}

// dA (+ its epilogue) and dW of one small-M backward layer in one launch; returns false (nothing launched) when the
// pair does not fit that form, and the caller launches the two separately.
bool try_launch_da_dw(const AOperand &dz, const BOperand &Win, int M, int Nout, int Kd, const Epilogue &Ein, int *nslab, const AOperand &a2,
                      int Kp, float *slab, int *nsplit_io, int *kp_pad_io, hipStream_t st, int *rc, float *dw_direct, int dw_ld) {
    *rc = PNPP_OK;
    Epilogue E = Ein;
    E.store_policy = store_policy();
    if (mid_tiles_on() && try_launch_mid_da_dw(dz, Win, M, Nout, Kd, E, nslab, a2, Kp, slab, nsplit_io, kp_pad_io, st, rc, dw_direct, dw_ld))
        return true;   // wide layers of a group_all level: 64 x 64 tiles over the whole reduction, no 64-row partials
    const int nsplit = *nsplit_io, kp_pad = *kp_pad_io;
    const int Nc = Kd;  // dZ is M x Nc; dA = dZ W contracts over Nc, dW is Nc x Kp
    if (!(M > 32 && M <= 4096 && cdiv(M, 32) <= kMaxStatBlocks && dz.mode == A_PLAIN && (dz.lda & 3) == 0 && ((uintptr_t)dz.a & 15) == 0))
        return false;
    if (!(Nc >= 128 && Kp >= 128 && Kd % 4 == 0 && !Win.trans && (E.mode == E_STORE || E.mode == E_MASK_STATS))) return false;
    if (!(a2.mode == A_PLAIN || a2.mode == A_BNRELU || a2.mode == A_CONCAT)) return false;
    if (a2.mode != A_CONCAT && ((a2.lda & 3) != 0 || ((uintptr_t)a2.a & 15) != 0)) return false;
    if (kp_pad != cdiv(Kp, 64) * 64 || nsplit < 1) return false;
    BOperand W = Win;
    if (W.rows <= 0 || W.rows > Kd) W.rows = Kd;
    const int g1x = cdiv(Nout, 32), g1y = cdiv(M, 32), g1 = g1x * g1y;
    const int tc = cdiv(Nc, 128), tk = cdiv(Kp, 128);
    int rps = cdiv(M, nsplit);
    rps = (rps + 7) & ~7;
    const dim3 grid(g1 + tc * tk * nsplit);
    if (nslab) *nslab = g1y;
    ProfScope ps(st, "da_dw_kernel<E%d,A%d> M=%d | dA N=%d K=%d grid=%d | dW N=%d K=%d split=%d grid=%d", E.mode, a2.mode, M, Nout, Kd, g1,
                 Nc, Kp, nsplit, tc * tk * nsplit);
#define PNPP_DADW(EM, AM) \
    hipLaunchKernelGGL((da_dw_kernel<EM, AM>), grid, dim3(256), 0, st, dz, W, M, Nout, Kd, E, g1x, g1, a2, Nc, Kp, tc, tk, rps, kp_pad, slab)
    if (E.mode == E_STORE) {
        if (a2.mode == A_PLAIN) PNPP_DADW(E_STORE, A_PLAIN);
        else if (a2.mode == A_BNRELU) PNPP_DADW(E_STORE, A_BNRELU);
        else PNPP_DADW(E_STORE, A_CONCAT);
    } else {
        if (a2.mode == A_PLAIN) PNPP_DADW(E_MASK_STATS, A_PLAIN);
        else if (a2.mode == A_BNRELU) PNPP_DADW(E_MASK_STATS, A_BNRELU);
        else PNPP_DADW(E_MASK_STATS, A_CONCAT);
    }
#undef PNPP_DADW
    check_launch("da_dw", rc);
    return true;
}

}  // namespace pnpp
