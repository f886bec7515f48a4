// symmetry_kernels.hip -- yaw symmetry of a cloud from its own geometry (include/pnpp_hip.h: pnpp_yaw_profile, pnpp_yaw_symmetry):
// the one-sided Chamfer distance between the cloud and its copy turned about +Y, at G angles, and the decision made from it.
//
// B * G * N^2 exact float32 distances and nothing else: VALU bound, no MFMA.  Candidates are staged in LDS once per workgroup, already
// centred, as 16-byte (x, y, z, -) rows; every lane of a wave reads the SAME row (one broadcast LDS read) and spends it on the
// PNPP_YAW_ANGLE_BLOCK rotated copies of its own query that it holds in registers.  Compiled with -ffp-contract=off, like the index
// kernels: the float32 steps are those of tests/symmetry_ref.py, one IEEE operation each.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

namespace pnpp {

constexpr int kYawA = PNPP_YAW_ANGLE_BLOCK;   // slots (rotations) a lane holds for its query
constexpr int kYawTile = PNPP_YAW_TILE;       // candidates staged per pass
constexpr int kYawQ = PNPP_YAW_QUERIES;       // queries per workgroup, one per lane
constexpr double kYawTwoPi = 6.283185307179586476925286766559;

// Slot s of a cloud: s = 0 is the floor (the identity rotation, a point is not its own candidate), s = 1 + g is angle g of the table.
// Workspace: part[b][qc][s] float64, s < yaw_slots(G), the sum of the minima of workgroup (b, qc)'s queries.
static inline int yaw_slot_blocks(int G) { return cdiv(G + 1, kYawA); }
static inline int yaw_slots(int G) { return yaw_slot_blocks(G) * kYawA; }
static inline int yaw_query_chunks(int N) { return cdiv(N, kYawQ); }
static size_t yaw_workspace_bytes(int B, int N, int G) { return (size_t)B * yaw_query_chunks(N) * yaw_slots(G) * sizeof(double); }

struct YawLds {
    float4 cand[kYawTile];
    double red[4][kYawA];
};

// One tile of candidates against a lane's query: min over j of exact_dist.h's direct_dist_exact(rot_a(q), cand_j), the lowest j among
// equals.  dy^2 does not depend on the rotation and is formed once per candidate; the other steps are direct_dist_exact's, in its order.
// FLOOR: slot 0 of this block is the floor, which leaves out candidate j == self.
template <bool NEAREST, bool FLOOR>
__device__ __forceinline__ void yaw_scan_tile(const YawLds &L, int count, int base, int self, float qy, const float (&rx)[kYawA],
                                              const float (&rz)[kYawA], float (&best)[kYawA], int (&arg)[kYawA]) {
#pragma unroll 2
    for (int j = 0; j < count; ++j) {
        const float4 c = L.cand[j];
        const float dy = __fsub_rn(qy, c.y);
        const float dy2 = __fmul_rn(dy, dy);
        const bool other = !FLOOR || (base + j != self);
#pragma unroll
        for (int a = 0; a < kYawA; ++a) {
            const float dx = __fsub_rn(rx[a], c.x), dz = __fsub_rn(rz[a], c.z);
            float d = __fmul_rn(dx, dx);
            d = __fadd_rn(d, dy2);
            d = __fadd_rn(d, __fmul_rn(dz, dz));
            if (a == 0 && FLOOR) d = other ? d : __builtin_inff();
            if (NEAREST) {
                const bool take = d < best[a];
                best[a] = take ? d : best[a];
                arg[a] = take ? base + j : arg[a];
            } else {
                best[a] = fminf(best[a], d);   // the same value as the compare-select above, in one instruction
            }
        }
    }
}

template <bool RAGGED, bool NEAREST, bool FLOOR>
__device__ __forceinline__ void yaw_profile_body(YawLds &L, const float *__restrict__ xyz, int N, const int32_t *__restrict__ lengths,
                                                 const float *__restrict__ centre, const float *__restrict__ table, int G,
                                                 double *__restrict__ part, float *__restrict__ ndist, int32_t *__restrict__ nidx) {
    const int sb = blockIdx.x, qc = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int nslots = gridDim.x * kYawA;
    int Nv = N;
    if (RAGGED) Nv = min(max(lengths[b], 1), N);
    const int i = qc * kYawQ + tid;
    const bool valid = i < Nv;
    const float *__restrict__ cloud = xyz + (size_t)b * N * 3;
    const float cx = centre[b * 3 + 0], cz = centre[b * 3 + 2];
    double *__restrict__ out = part + ((size_t)b * gridDim.y + qc) * nslots + sb * kYawA;

    // the slots of this block: their table rows, the query turned by each
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (valid) {
        qx = __fsub_rn(cloud[(size_t)i * 3 + 0], cx);
        qy = cloud[(size_t)i * 3 + 1];
        qz = __fsub_rn(cloud[(size_t)i * 3 + 2], cz);
    }
    float rx[kYawA], rz[kYawA], best[kYawA];
    int arg[kYawA];
#pragma unroll
    for (int a = 0; a < kYawA; ++a) {
        const int g = sb * kYawA + a - 1;   // -1: the floor; >= G: past the table, computed as the identity and never written
        float cs = 1.0f, sn = 0.0f;
        if (g >= 0 && g < G) cs = table[g * 2 + 0], sn = table[g * 2 + 1];
        rx[a] = __fadd_rn(__fmul_rn(cs, qx), __fmul_rn(sn, qz));
        rz[a] = __fsub_rn(__fmul_rn(cs, qz), __fmul_rn(sn, qx));
        best[a] = __builtin_inff();
        arg[a] = -1;
    }

    if (qc * kYawQ < Nv) {   // the same in every lane of the workgroup: a chunk of padding rows scans nothing
        for (int t0 = 0; t0 < Nv; t0 += kYawTile) {
            const int count = min(kYawTile, Nv - t0);
            __syncthreads();   // the previous tile has been scanned
            for (int j = tid; j < count; j += kYawQ) {
                const float *__restrict__ p = cloud + (size_t)(t0 + j) * 3;
                L.cand[j] = make_float4(__fsub_rn(p[0], cx), p[1], __fsub_rn(p[2], cz), 0.0f);
            }
            __syncthreads();
            yaw_scan_tile<NEAREST, FLOOR>(L, count, t0, i, qy, rx, rz, best, arg);
        }
    }

    // float64 sums in a fixed order: the lanes of a wave (butterfly), then the four waves
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int a = 0; a < kYawA; ++a) {
        const bool none = !valid || (FLOOR && a == 0 && Nv == 1);   // a padding query; the floor of a cloud of one point
        double s = none ? 0.0 : (double)best[a];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += shfl_xor_f64(s, m);
        if (lane == 0) L.red[wave][a] = s;
    }
    __syncthreads();
    if (tid < kYawA) out[tid] = ((L.red[0][tid] + L.red[1][tid]) + L.red[2][tid]) + L.red[3][tid];

    if (NEAREST && i < N) {
#pragma unroll
        for (int a = 0; a < kYawA; ++a) {
            const int g = sb * kYawA + a - 1;
            if (g < 0 || g >= G) continue;
            const size_t o = ((size_t)b * G + g) * N + i;
            ndist[o] = valid ? best[a] : 0.0f;
            nidx[o] = valid ? arg[a] : -1;
        }
    }
}

// grid (slot blocks, query chunks, B), 256 threads.  Slot block 0 carries the floor.
template <bool RAGGED, bool NEAREST>
__global__ void __launch_bounds__(256) yaw_profile_kernel(const float *__restrict__ xyz, int N, const int32_t *__restrict__ lengths,
                                                          const float *__restrict__ centre, const float *__restrict__ table, int G,
                                                          double *__restrict__ part, float *__restrict__ ndist,
                                                          int32_t *__restrict__ nidx) {
    __shared__ YawLds L;
    if (blockIdx.x == 0) yaw_profile_body<RAGGED, NEAREST, true>(L, xyz, N, lengths, centre, table, G, part, ndist, nidx);
    else yaw_profile_body<RAGGED, NEAREST, false>(L, xyz, N, lengths, centre, table, G, part, ndist, nidx);
}

struct YawOrders {
    int n;
    int m[PNPP_YAW_MAX_ORDERS];
};

// The mean of slot s over the cloud's valid queries: the query chunks' partial sums in chunk order, float64, rounded once.
__device__ __forceinline__ float yaw_mean(const double *__restrict__ part, int nq, int nslots, int s, int Nv) {
    double t = 0.0;
    for (int q = 0; q < nq; ++q) t += part[(size_t)q * nslots + s];
    return (float)(t / (double)Nv);
}

// One wave per cloud: D and nu from the partial sums, S[g] = D[g] + D[(G - g) % G], score = S / (2 nu), and the decision.
__global__ void __launch_bounds__(64) yaw_symmetry_kernel(const double *__restrict__ part, int N, const int32_t *__restrict__ lengths, int G,
                                                          float tol, const YawOrders orders, float *__restrict__ distance,
                                                          float *__restrict__ floor_out, float *__restrict__ score,
                                                          int32_t *__restrict__ order_out, int32_t *__restrict__ count_out,
                                                          float *__restrict__ angles, int angle_stride) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nq = (N + kYawQ - 1) / kYawQ, nslots = (G + 1 + kYawA - 1) / kYawA * kYawA;
    const int Nv = lengths ? min(max(lengths[b], 1), N) : N;
    const double *__restrict__ mine = part + (size_t)b * nq * nslots;
    const float nu = yaw_mean(mine, nq, nslots, 0, Nv);
    const float twonu = __fmul_rn(2.0f, nu);
    const float bound = __fmul_rn(twonu, tol);
    if (lane == 0) floor_out[b] = nu;
    const bool decide = order_out != nullptr;

    bool all_within = true;   // S[g] <= bound for every g >= 1 this lane has seen
    for (int g = lane; g < G; g += 64) {
        const float d = yaw_mean(mine, nq, nslots, 1 + g, Nv);
        distance[(size_t)b * G + g] = d;
        if (!decide) continue;
        const float s = __fadd_rn(d, yaw_mean(mine, nq, nslots, 1 + (G - g) % G, Nv));
        score[(size_t)b * G + g] = __fdiv_rn(s, twonu);
        if (g >= 1 && !(s <= bound)) all_within = false;
    }
    if (!decide) return;

    int order = 1;
    if (__all(all_within)) {
        order = 0;
    } else {
        for (int t = 0; t < orders.n; ++t) {   // the largest admitted order whose every rotation maps the cloud onto itself
            const int m = orders.m[t];
            if (m <= order) continue;
            const int step = G / m;
            bool ok = true;
            for (int k = 1 + lane; k < m; k += 64) {
                const int g = k * step;
                const float s = __fadd_rn(yaw_mean(mine, nq, nslots, 1 + g, Nv), yaw_mean(mine, nq, nslots, 1 + (G - g) % G, Nv));
                if (!(s <= bound)) ok = false;
            }
            if (__all(ok)) order = m;
        }
    }
    if (lane == 0) order_out[b] = order, count_out[b] = order;
    for (int k = lane; k < angle_stride; k += 64)
        angles[(size_t)b * angle_stride + k] = k < order ? (float)(kYawTwoPi * (double)k / (double)order) : 0.0f;
}

// ---------------------------------------------------------------------------------------------
// host launchers.  Every refusal comes before any launch.
// ---------------------------------------------------------------------------------------------
static int launch_yaw_profile(const float *xyz, int B, int N, const int32_t *lengths, const float *centre, const float *table, int G,
                              void *workspace, size_t workspace_bytes, float *ndist, int32_t *nidx, hipStream_t st) {
    PNPP_REQUIRE(xyz && centre && table && workspace, PNPP_ERR_ARG, "yaw_profile: null pointer");
    PNPP_REQUIRE((ndist == nullptr) == (nidx == nullptr), PNPP_ERR_ARG, "yaw_profile: nearest distances and indices come together");
    PNPP_REQUIRE(B >= 1 && N >= 1, PNPP_ERR_ARG, "yaw_profile: non-positive size (B=%d N=%d)", B, N);
    PNPP_REQUIRE(G >= 1, PNPP_ERR_ARG, "yaw_profile: non-positive number of angles (G=%d)", G);
    PNPP_REQUIRE(B <= 65535 && yaw_query_chunks(N) <= 65535, PNPP_ERR_ARG, "yaw_profile: B=%d N=%d exceeds grid limit", B, N);
    PNPP_REQUIRE(workspace_bytes >= yaw_workspace_bytes(B, N, G), PNPP_ERR_ARG, "yaw_profile: workspace too small (%zu bytes, %zu needed)",
                 workspace_bytes, yaw_workspace_bytes(B, N, G));
    ProfScope ps(st, "yaw_profile_kernel B=%d N=%d G=%d%s%s", B, N, G, lengths ? " ragged" : "", ndist ? " +nearest" : "");
    const dim3 grid(yaw_slot_blocks(G), yaw_query_chunks(N), B);
    const auto kfn = lengths ? (ndist ? yaw_profile_kernel<true, true> : yaw_profile_kernel<true, false>)
                             : (ndist ? yaw_profile_kernel<false, true> : yaw_profile_kernel<false, false>);
    hipLaunchKernelGGL(kfn, grid, dim3(256), 0, st, xyz, N, lengths, centre, table, G, static_cast<double *>(workspace), ndist, nidx);
    PNPP_CHECK_LAUNCH("yaw_profile");
    return PNPP_OK;
}

}  // namespace pnpp

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace pnpp;

extern "C" size_t pnpp_yaw_workspace_bytes(int B, int N, int G) {
    if (B < 1 || N < 1 || G < 1) {
        set_error("yaw_workspace_bytes: non-positive size (B=%d N=%d G=%d)", B, N, G);
        return 0;
    }
    return yaw_workspace_bytes(B, N, G);
}

extern "C" int pnpp_yaw_profile(const float *xyz, int B, int N, const float *centre, const float *table, int G, void *workspace,
                                size_t workspace_bytes, float *nearest_dist, int32_t *nearest_idx, void *stream) {
    return launch_yaw_profile(xyz, B, N, nullptr, centre, table, G, workspace, workspace_bytes, nearest_dist, nearest_idx, as_stream(stream));
}

extern "C" int pnpp_yaw_profile_ragged(const float *xyz, int B, int N, const int32_t *lengths, const float *centre, const float *table,
                                       int G, void *workspace, size_t workspace_bytes, float *nearest_dist, int32_t *nearest_idx,
                                       void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "yaw_profile_ragged: null lengths");
    return launch_yaw_profile(xyz, B, N, lengths, centre, table, G, workspace, workspace_bytes, nearest_dist, nearest_idx, as_stream(stream));
}

extern "C" int pnpp_yaw_symmetry(const void *workspace, size_t workspace_bytes, int B, int N, const int32_t *lengths, int G, float tol,
                                 const int32_t *orders, int n_orders, float *distance, float *floor, float *score, int32_t *order,
                                 int32_t *count, float *angles, int angle_stride, void *stream) {
    PNPP_REQUIRE(workspace && distance && floor, PNPP_ERR_ARG, "yaw_symmetry: null pointer");
    PNPP_REQUIRE(B >= 1 && N >= 1, PNPP_ERR_ARG, "yaw_symmetry: non-positive size (B=%d N=%d)", B, N);
    PNPP_REQUIRE(G >= 1, PNPP_ERR_ARG, "yaw_symmetry: non-positive number of angles (G=%d)", G);
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "yaw_symmetry: B=%d exceeds grid limit", B);
    PNPP_REQUIRE(workspace_bytes >= yaw_workspace_bytes(B, N, G), PNPP_ERR_ARG, "yaw_symmetry: workspace too small (%zu bytes, %zu needed)",
                 workspace_bytes, yaw_workspace_bytes(B, N, G));
    YawOrders O{0, {0}};
    const bool decide = score || order || count || angles;   // none of them: the profile alone is finished
    if (decide) {
        PNPP_REQUIRE(score && order && count && angles, PNPP_ERR_ARG, "yaw_symmetry: null pointer");
        PNPP_REQUIRE(std::isfinite(tol) && tol >= 0.0f, PNPP_ERR_ARG, "yaw_symmetry: tol=%g is not a finite, non-negative number", (double)tol);
        PNPP_REQUIRE(n_orders >= 0 && n_orders <= PNPP_YAW_MAX_ORDERS && (n_orders == 0 || orders), PNPP_ERR_ARG,
                     "yaw_symmetry: %d candidate orders (at most %d, with their list)", n_orders, PNPP_YAW_MAX_ORDERS);
        int largest = 1;
        for (int t = 0; t < n_orders; ++t) {
            PNPP_REQUIRE(orders[t] >= 2, PNPP_ERR_ARG, "yaw_symmetry: candidate order %d is below 2", orders[t]);
            PNPP_REQUIRE(G % orders[t] == 0, PNPP_ERR_ARG, "yaw_symmetry: candidate order %d does not divide G=%d", orders[t], G);
            O.m[t] = orders[t];
            largest = orders[t] > largest ? orders[t] : largest;
        }
        O.n = n_orders;
        PNPP_REQUIRE(angle_stride >= largest, PNPP_ERR_ARG, "yaw_symmetry: angle stride %d is below the largest candidate order %d",
                     angle_stride, largest);
    }
    hipStream_t st = as_stream(stream);
    ProfScope ps(st, "yaw_symmetry_kernel B=%d N=%d G=%d%s", B, N, G, decide ? " +decision" : "");
    hipLaunchKernelGGL(yaw_symmetry_kernel, dim3(B), dim3(64), 0, st, static_cast<const double *>(workspace), N, lengths, G, tol, O, distance,
                       floor, score, order, count, angles, angle_stride);
    PNPP_CHECK_LAUNCH("yaw_symmetry");
    return PNPP_OK;
}
