// group_kernels.hip -- grouping for gfx950 (MI355X): square_distance, the radius ball query, the row gather and its backward scatter,
// and the centre gather; their launchers and C entries.  Copy- or compare-bound, no MFMA.
// Compiled with -ffp-contract=off (exact_dist.h): the distances are the reference's exact float32 sequences.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "exact_dist.h"

namespace pnpp {

// ---------------------------------------------------------------------------------------------
// square_distance: one thread per output element, n fastest (coalesced 4-byte stores)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) square_distance_kernel(const float *__restrict__ src,
                                                              const float *__restrict__ dst, int S, int N,
                                                              float *__restrict__ out) {
    const int b = blockIdx.z, s = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float *a = src + ((size_t)b * S + s) * 3;
    const float *q = dst + ((size_t)b * N + n) * 3;
    const float ax = a[0], ay = a[1], az = a[2];
    const float bx = q[0], by = q[1], bz = q[2];
    out[((size_t)b * S + s) * N + n] = pair_dist_exact(ax, ay, az, bx, by, bz, sq3_exact(ax, ay, az), sq3_exact(bx, by, bz));
}

// ---------------------------------------------------------------------------------------------
// radius ball query (PointNet++Demo.py:49-70): one wavefront per centre, ascending index scan,
// ballot + prefix popcount compaction, early exit once nsample hits were written.
// ---------------------------------------------------------------------------------------------
constexpr int BALL_TILE = 1024;   // candidates staged per step (x, y, z: 12 KiB)

// RAGGED: the scan covers the cloud's own rows < Nv = min(max(lengths[b], 1), N), and a centre without a member is filled with Nv.
template <bool RAGGED>
__global__ void __launch_bounds__(256) ball_query_kernel(const float *__restrict__ new_xyz, const float *__restrict__ xyz,
                                                         int S, const int Npad, float r2, int nsample, int32_t *__restrict__ idx,
                                                         const int32_t *__restrict__ lengths) {
    __shared__ float sx[BALL_TILE], sy[BALL_TILE], sz[BALL_TILE];
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    const bool active = q < S;
    float ax = 0.f, ay = 0.f, az = 0.f;
    int32_t *o = nullptr;
    if (active) {
        const float *a = new_xyz + ((size_t)b * S + q) * 3;
        ax = a[0], ay = a[1], az = a[2];
        o = idx + ((size_t)b * S + q) * nsample;
    }
    int N = Npad;
    if constexpr (RAGGED) N = min(max(lengths[b], 1), Npad);
    int cnt = 0, first = N;  // wave-uniform
    const float *cloud = xyz + (size_t)b * Npad * 3;
    for (int t0 = 0; t0 < N; t0 += BALL_TILE) {
        __syncthreads();
        const int tc = min(BALL_TILE, N - t0);
        for (int i = threadIdx.x; i < tc * 3; i += 256) {
            float v = cloud[(size_t)t0 * 3 + i];
            int p = i / 3, c = i - p * 3;
            (c == 0 ? sx : c == 1 ? sy : sz)[p] = v;
        }
        __syncthreads();
        if (!active || cnt >= nsample) continue;
        for (int c0 = 0; c0 < tc && cnt < nsample; c0 += 64) {
            const int p = c0 + lane;
            bool in = false;
            if (p < tc) {
                float d = direct_dist_exact(ax, ay, az, sx[p], sy[p], sz[p]);
                in = !(d > r2);
            }
            const unsigned long long m = __ballot(in);
            if (m == 0ull) continue;
            if (first == N) first = t0 + c0 + (__ffsll((long long)m) - 1);
            const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
            if (in && pos < nsample) o[pos] = t0 + p;
            cnt += __popcll(m);
        }
    }
    if (active) {
        cnt = min(cnt, nsample);
        for (int j = cnt + lane; j < nsample; j += 64) o[j] = first;
    }
}

// ---------------------------------------------------------------------------------------------
// index_points (models/base.py:4-18): row gather, 16-byte vectors when C % 4 == 0
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gather_rows_kernel(const float *__restrict__ points, const int32_t *__restrict__ idx,
                                                          int N, int C, int M, size_t total_vec, int vec,
                                                          float *__restrict__ out) {
    const int cv = C / vec;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total_vec; i += (size_t)gridDim.x * 256) {
        const size_t row = i / cv;
        const int c = (int)(i - row * cv) * vec;
        const int b = (int)(row / M);
        const int n = idx[row];
        const float *s = points + ((size_t)b * N + n) * C + c;
        float *d = out + row * C + c;
        if (vec == 4) {
            *reinterpret_cast<float4 *>(d) = *reinterpret_cast<const float4 *>(s);
        } else {
            *d = *s;
        }
    }
}

// backward of the gather: one wavefront per destination row (b,n); the cloud's M indices are scanned
// in order, so duplicate contributions are added in a fixed order (bitwise reproducible, no atomics).
__global__ void __launch_bounds__(64) scatter_rows_bwd_kernel(const float *__restrict__ dout, const int32_t *__restrict__ idx,
                                                              int N, int C, int M, float *__restrict__ dpoints) {
    const int b = blockIdx.y, n = blockIdx.x, lane = threadIdx.x;
    const int32_t *ib = idx + (size_t)b * M;
    const float *db = dout + (size_t)b * M * C;
    for (int c0 = 0; c0 < C; c0 += 64 * 8) {
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        for (int m0 = 0; m0 < M; m0 += 64) {
            const int m = m0 + lane;
            unsigned long long hit = __ballot(m < M && ib[m] == n);
            while (hit) {
                const int p = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                const float *r = db + (size_t)(m0 + p) * C + c0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = j * 64 + lane;
                    if (c0 + c < C) acc[j] += r[c];
                }
            }
        }
        float *d = dpoints + ((size_t)b * N + n) * C + c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = j * 64 + lane;
            if (c0 + c < C) d[c] += acc[j];
        }
    }
}

// gather of centre coordinates new_xyz[b,s,:] = xyz[b, centre[b,s], :] into two destinations (the caller's output and
// the copy kept for backward); centre == nullptr writes the origin (group_all, pointnet_pp_8dir.py:24)
__global__ void __launch_bounds__(256) gather_centres_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ centre,
                                                             int N, int S, int total, float *__restrict__ out_a,
                                                             float *__restrict__ out_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float x = 0.f, y = 0.f, z = 0.f;
    if (centre) {
        const int b = i / S;
        const float *s = xyz + ((size_t)b * N + centre[i]) * 3;
        x = s[0], y = s[1], z = s[2];
    }
    out_a[(size_t)i * 3 + 0] = x;
    out_a[(size_t)i * 3 + 1] = y;
    out_a[(size_t)i * 3 + 2] = z;
    if (out_b) {
        out_b[(size_t)i * 3 + 0] = x;
        out_b[(size_t)i * 3 + 1] = y;
        out_b[(size_t)i * 3 + 2] = z;
    }
}

// ---------------------------------------------------------------------------------------------
// host launchers (internal C++ API, used by the C ABI and by the set-abstraction orchestrator)
// ---------------------------------------------------------------------------------------------
int launch_gather_centres(const float *xyz, const int32_t *centre, int B, int N, int S, float *out_a, float *out_b,
                          hipStream_t st) {
    const int total = B * S;
    ProfScope ps(st, "gather_centres_kernel B=%d S=%d", B, S);
    hipLaunchKernelGGL(gather_centres_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, xyz, centre, N, S, total, out_a, out_b);
    PNPP_CHECK_LAUNCH("gather_centres");
    return PNPP_OK;
}

int launch_scatter_rows_bwd(const float *dout, const int32_t *idx, int B, int N, int C, int M, float *dpoints, hipStream_t st) {
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "index_points_bwd: batch %d exceeds grid limit", B);
    ProfScope ps(st, "scatter_rows_bwd_kernel B=%d N=%d C=%d M=%d", B, N, C, M);
    hipLaunchKernelGGL(scatter_rows_bwd_kernel, dim3(N, B), dim3(64), 0, st, dout, idx, N, C, M, dpoints);
    PNPP_CHECK_LAUNCH("index_points_bwd");
    return PNPP_OK;
}

}  // namespace pnpp

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace pnpp;

extern "C" int pnpp_square_distance(const float *src, const float *dst, int B, int S, int N, float *out, void *stream) {
    PNPP_REQUIRE(src && dst && out, PNPP_ERR_ARG, "square_distance: null pointer");
    PNPP_REQUIRE(B > 0 && S > 0 && N > 0, PNPP_ERR_ARG, "square_distance: non-positive size");
    PNPP_REQUIRE(B <= 65535 && S <= 65535, PNPP_ERR_ARG, "square_distance: B or S exceeds grid limit");
    hipLaunchKernelGGL(square_distance_kernel, dim3(cdiv(N, 256), S, B), dim3(256), 0, as_stream(stream), src, dst, S, N, out);
    PNPP_CHECK_LAUNCH("square_distance");
    return PNPP_OK;
}

// r2 is the float32 threshold the kernel compares against: a member is a point with !(d > r2).
static int ball_query_impl(const float *new_xyz, const float *xyz, int B, int S, int N, const int32_t *lengths, float r2, int nsample,
                           int32_t *idx, void *stream) {
    PNPP_REQUIRE(new_xyz && xyz && idx, PNPP_ERR_ARG, "ball_query: null pointer");
    PNPP_REQUIRE(B > 0 && S > 0 && N > 0 && nsample > 0, PNPP_ERR_ARG, "ball_query: non-positive size");
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "ball_query: batch exceeds grid limit");
    ProfScope ps(as_stream(stream), "ball_query_kernel B=%d S=%d N=%d nsample=%d%s", B, S, N, nsample, lengths ? " ragged" : "");
    const auto kfn = lengths ? ball_query_kernel<true> : ball_query_kernel<false>;
    hipLaunchKernelGGL(kfn, dim3(cdiv(S, 4), B), dim3(256), 0, as_stream(stream), new_xyz, xyz, S, N, r2, nsample, idx, lengths);
    PNPP_CHECK_LAUNCH("ball_query");
    return PNPP_OK;
}

// A float radius squared in double and rounded: the radius has been rounded to float32 before it is squared, so for most radii this
// is NOT float32(radius ** 2) of the python float the reference squares (Demo.py:65).  The _r2 entries take that value as it is.
static float r2_of_float_radius(float radius) { return (float)((double)radius * (double)radius); }

extern "C" int pnpp_ball_query(const float *new_xyz, const float *xyz, int B, int S, int N, float radius, int nsample,
                               int32_t *idx, void *stream) {
    return ball_query_impl(new_xyz, xyz, B, S, N, nullptr, r2_of_float_radius(radius), nsample, idx, stream);
}
extern "C" int pnpp_ball_query_ragged(const float *new_xyz, const float *xyz, int B, int S, int N, const int32_t *lengths, float radius,
                                      int nsample, int32_t *idx, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "ball_query_ragged: null lengths");
    return ball_query_impl(new_xyz, xyz, B, S, N, lengths, r2_of_float_radius(radius), nsample, idx, stream);
}
extern "C" int pnpp_ball_query_r2(const float *new_xyz, const float *xyz, int B, int S, int N, float r2, int nsample, int32_t *idx,
                                  void *stream) {
    return ball_query_impl(new_xyz, xyz, B, S, N, nullptr, r2, nsample, idx, stream);
}
extern "C" int pnpp_ball_query_r2_ragged(const float *new_xyz, const float *xyz, int B, int S, int N, const int32_t *lengths, float r2,
                                         int nsample, int32_t *idx, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "ball_query_r2_ragged: null lengths");
    return ball_query_impl(new_xyz, xyz, B, S, N, lengths, r2, nsample, idx, stream);
}

extern "C" int pnpp_index_points(const float *points, const int32_t *idx, int B, int N, int C, int M, float *out, void *stream) {
    PNPP_REQUIRE(points && idx && out, PNPP_ERR_ARG, "index_points: null pointer");
    PNPP_REQUIRE(B > 0 && N > 0 && C > 0 && M > 0, PNPP_ERR_ARG, "index_points: non-positive size");
    const int vec = (C % 4 == 0 && ((uintptr_t)points % 16 == 0) && ((uintptr_t)out % 16 == 0)) ? 4 : 1;
    const size_t total = (size_t)B * M * (C / vec);
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(256), 0, as_stream(stream), points, idx, N, C, M, total, vec, out);
    PNPP_CHECK_LAUNCH("index_points");
    return PNPP_OK;
}

extern "C" int pnpp_index_points_bwd(const float *dout, const int32_t *idx, int B, int N, int C, int M, float *dpoints,
                                     void *stream) {
    PNPP_REQUIRE(dout && idx && dpoints, PNPP_ERR_ARG, "index_points_bwd: null pointer");
    PNPP_REQUIRE(B > 0 && N > 0 && C > 0 && M > 0, PNPP_ERR_ARG, "index_points_bwd: non-positive size");
    return launch_scatter_rows_bwd(dout, idx, B, N, C, M, dpoints, as_stream(stream));
}
