// augment_kernels.hip -- training-time augmentation of a device-resident batch for gfx950 (MI355X): one yaw about +Y per
// cloud, optionally a scale and a clipped Gaussian jitter per point, and the orientation targets moved along -- one launch.
//
// Memory-bound: one pass over B N C floats.  A workgroup stages its tile of 256 rows (256 C contiguous floats) through LDS so
// that the global accesses are contiguous across the lanes (16 bytes per lane where the tile bases are 16-byte aligned, 4
// otherwise) while each thread works on one row; the LDS row stride is C = 3 dwords (conflict-free) or 6 (two-way).
//
// Reproducibility: every float32 step is an IEEE basic operation in a fixed order (this file is compiled with
// -ffp-contract=off and spells the operations out), the per-cloud and jitter values are float64 rounded once.
// tests/augment_ref.py is the CPU restatement.
#include "common.h"
#include "sampler_device.h"

#pragma clang fp contract(off)

namespace pnpp {

constexpr int kAugTile = 256;
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kPi = 3.141592653589793238462643383280;
constexpr double kTwoPiOver2p32 = kTwoPi / 4294967296.0;   // exact: a power-of-two division

struct AugCloud {
    float c, s, scale;
    double theta;
};

// x' = fl(fl(c x) + fl(s z)), z' = fl(fl(c z) - fl(s x)): rows p' = p R^T with R = [[c,0,s],[0,1,0],[-s,0,c]]
__device__ __forceinline__ void yaw_rotate(const AugCloud &a, float &x, float &z) {
    const float xo = __fadd_rn(__fmul_rn(a.c, x), __fmul_rn(a.s, z));
    const float zo = __fsub_rn(__fmul_rn(a.c, z), __fmul_rn(a.s, x));
    x = xo, z = zo;
}

__device__ __forceinline__ AugCloud aug_cloud_params(const pnpp_augment_desc &d, unsigned b, unsigned str_lo, unsigned str_hi,
                                                     unsigned seed_lo, unsigned seed_hi) {
    AugCloud a{1.0f, 0.0f, 1.0f, 0.0};
    if (!(d.flags & (PNPP_AUG_YAW | PNPP_AUG_SCALE))) return a;
    const uint4 w = philox4(0xFFFFFFFFu, b, str_lo, str_hi, seed_lo, seed_hi);
    if (d.flags & PNPP_AUG_YAW) {
        a.theta = (double)w.x * kTwoPiOver2p32;
        a.c = (float)cos(a.theta);
        a.s = (float)sin(a.theta);
    }
    if (d.flags & PNPP_AUG_SCALE) {
        const double lo = (double)d.scale_lo, hi = (double)d.scale_hi;
        a.scale = (float)(lo + (hi - lo) * ((double)w.y * (1.0 / 4294967296.0)));
    }
    return a;
}

// mu' = (float) wrap((double) mu - theta): mu in (-pi, pi], theta in [0, 2 pi), so one conditional + 2 pi
__device__ __forceinline__ float shift_angle(float mu, double theta) {
    double v = (double)mu - theta;
    if (v <= -kPi) v += kTwoPi;
    return (float)v;
}

// one Box-Muller pair from two words: u = (w + 1) / 2^32 in (0, 1]
__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, double &z0, double &z1) {
    const double u = ((double)wa + 1.0) * (1.0 / 4294967296.0);
    const double r = sqrt(-2.0 * log(u));
    const double ang = (double)wb * kTwoPiOver2p32;
    z0 = r * cos(ang);
    z1 = r * sin(ang);
}

__device__ __forceinline__ float jitter_value(double z, double sigma, double clip) {
    double j = sigma * z;
    j = j < -clip ? -clip : (j > clip ? clip : j);
    return (float)j;
}

// the targets of cloud b: block x = 0 only
__device__ __forceinline__ void augment_targets(const pnpp_augment_desc &d, const AugCloud &a, int b) {
    const bool yaw = (d.flags & PNPP_AUG_YAW) != 0;
    for (int t = 0; t < d.n_targets; ++t) {
        const pnpp_augment_target &g = d.targets[t];
        const int count = g.counts ? min(max(g.counts[b], 0), g.rows) : g.rows;
        if (g.kind == PNPP_AUG_ANGLE || g.kind == PNPP_AUG_VM) {
            const int cols = g.cols, n = g.rows * cols;
            const float *__restrict__ in = g.in + (size_t)b * n;
            float *__restrict__ out = g.out + (size_t)b * n;
            for (int e = threadIdx.x; e < n; e += kAugTile) {
                const int row = e / cols, col = e - row * cols;
                const float v = in[e];
                out[e] = (yaw && col == 0 && row < count) ? shift_angle(v, a.theta) : v;
            }
        } else if (g.kind == PNPP_AUG_AXIS) {
            const float *__restrict__ in = g.in + (size_t)b * g.rows * 3;
            float *__restrict__ out = g.out + (size_t)b * g.rows * 3;
            for (int r = threadIdx.x; r < g.rows; r += kAugTile) {
                float x = in[r * 3 + 0], y = in[r * 3 + 1], z = in[r * 3 + 2];
                if (yaw && r < count) yaw_rotate(a, x, z);
                out[r * 3 + 0] = x, out[r * 3 + 1] = y, out[r * 3 + 2] = z;
            }
        } else if (threadIdx.x == 0) {   // DIR8: eight values per cloud, summed in order
            const float *__restrict__ in = g.in + (size_t)b * 3;
            float *__restrict__ out = g.out + (size_t)b * 8;
            float x = in[0], y = in[1], z = in[2];
            if (yaw && count > 0) yaw_rotate(a, x, z);
            float r[8], sum = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float dot = __fadd_rn(__fadd_rn(__fmul_rn(d.dirs8[i * 3 + 0], x), __fmul_rn(d.dirs8[i * 3 + 1], y)),
                                            __fmul_rn(d.dirs8[i * 3 + 2], z));
                r[i] = dot > 0.0f ? dot : 0.0f;
                sum = __fadd_rn(sum, r[i]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) out[i] = sum == 0.0f ? 0.125f : __fdiv_rn(r[i], sum);
        }
    }
}

// grid (point tiles, B), 256 threads.  VEC = 4: every tile base is 16-byte aligned (N C a multiple of 4, aligned pointers).
template <int VEC>
__global__ __launch_bounds__(kAugTile) void augment_clouds_kernel(unsigned seed_lo, unsigned seed_hi, unsigned str_lo, unsigned str_hi,
                                                                  const float *__restrict__ xyz_in, float *__restrict__ xyz_out,
                                                                  const int32_t *__restrict__ lengths, long long N, int C,
                                                                  pnpp_augment_desc d, float *__restrict__ params) {
    __shared__ __attribute__((aligned(16))) float tile[kAugTile * 6];
    const int b = blockIdx.y;
    const long long n0 = (long long)blockIdx.x * kAugTile;
    const int np = (int)min((long long)kAugTile, N - n0);   // rows of this tile
    const int nf = np * C;                                  // floats of this tile (VEC = 4: a multiple of 4)
    const size_t base = ((size_t)b * (size_t)N + (size_t)n0) * (size_t)C;
    for (int i = threadIdx.x * VEC; i < nf; i += kAugTile * VEC) {
        if constexpr (VEC == 4)
            *reinterpret_cast<float4 *>(&tile[i]) = *reinterpret_cast<const float4 *>(&xyz_in[base + i]);
        else
            tile[i] = xyz_in[base + i];
    }
    const AugCloud a = aug_cloud_params(d, (unsigned)b, str_lo, str_hi, seed_lo, seed_hi);
    long long nv = N;
    if (lengths) nv = min(max((long long)lengths[b], 0ll), N);
    __syncthreads();
    const long long n = n0 + threadIdx.x;
    if ((int)threadIdx.x < np && n < nv) {
        float *p = &tile[threadIdx.x * C];
        float x = p[0], y = p[1], z = p[2];
        if (d.flags & PNPP_AUG_YAW) {
            yaw_rotate(a, x, z);
            if (C == 6) {
                float nx = p[3], nz = p[5];
                yaw_rotate(a, nx, nz);
                p[3] = nx, p[5] = nz;
            }
        }
        if (d.flags & PNPP_AUG_SCALE) x = __fmul_rn(x, a.scale), y = __fmul_rn(y, a.scale), z = __fmul_rn(z, a.scale);
        if (d.flags & PNPP_AUG_JITTER) {
            const uint4 w = philox4((unsigned)n, (unsigned)b, str_lo, str_hi, seed_lo, seed_hi);
            double z0, z1, z2, z3;
            box_muller(w.x, w.y, z0, z1);
            box_muller(w.z, w.w, z2, z3);
            const double sg = (double)d.sigma, cl = (double)d.clip;
            x = __fadd_rn(x, jitter_value(z0, sg, cl));
            y = __fadd_rn(y, jitter_value(z1, sg, cl));
            z = __fadd_rn(z, jitter_value(z2, sg, cl));
        }
        p[0] = x, p[1] = y, p[2] = z;
    }
    __syncthreads();
    for (int i = threadIdx.x * VEC; i < nf; i += kAugTile * VEC) {
        if constexpr (VEC == 4)
            *reinterpret_cast<float4 *>(&xyz_out[base + i]) = *reinterpret_cast<const float4 *>(&tile[i]);
        else
            xyz_out[base + i] = tile[i];
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {
            float *q = params + (size_t)b * 4;
            q[0] = a.c, q[1] = a.s, q[2] = a.scale, q[3] = (float)a.theta;
        }
        augment_targets(d, a, b);
    }
}

}  // namespace pnpp

using namespace pnpp;

extern "C" int pnpp_augment_clouds(uint64_t seed, uint64_t stream_id, const float *xyz_in, float *xyz_out, const int32_t *lengths, int B,
                                   int64_t N, int C, const pnpp_augment_desc *desc, float *params_out, void *stream) {
    PNPP_REQUIRE(xyz_in && xyz_out && desc && params_out, PNPP_ERR_ARG, "augment_clouds: null pointer");
    PNPP_REQUIRE(B > 0 && B <= 65535 && N > 0, PNPP_ERR_ARG, "augment_clouds: B must be 1..65535 and N positive (B=%d N=%lld)", B,
                 (long long)N);
    PNPP_REQUIRE(N < 0xFFFFFFFFll, PNPP_ERR_ARG, "augment_clouds: N=%lld: the point counter is 32 bits and 2^32 - 1 is the cloud's own",
                 (long long)N);
    PNPP_REQUIRE(C == 3 || C == 6, PNPP_ERR_ARG, "augment_clouds: C=%d: rows are xyz (3) or xyz + normal (6)", C);
    PNPP_REQUIRE(xyz_in != xyz_out, PNPP_ERR_ARG, "augment_clouds: out of place only (xyz_in == xyz_out)");
    const pnpp_augment_desc &d = *desc;
    PNPP_REQUIRE(!(d.flags & ~(PNPP_AUG_YAW | PNPP_AUG_SCALE | PNPP_AUG_JITTER)), PNPP_ERR_ARG, "augment_clouds: unknown flag bits 0x%x",
                 d.flags);
    if (d.flags & PNPP_AUG_SCALE)
        PNPP_REQUIRE(d.scale_lo > 0.0f && d.scale_lo <= d.scale_hi && d.scale_hi < INFINITY, PNPP_ERR_ARG,
                     "augment_clouds: scale range must satisfy 0 < lo <= hi (lo=%g hi=%g)", (double)d.scale_lo, (double)d.scale_hi);
    if (d.flags & PNPP_AUG_JITTER)
        PNPP_REQUIRE(d.sigma >= 0.0f && d.sigma < INFINITY && d.clip >= 0.0f, PNPP_ERR_ARG,
                     "augment_clouds: jitter needs sigma >= 0 and clip >= 0 (sigma=%g clip=%g)", (double)d.sigma, (double)d.clip);
    PNPP_REQUIRE(d.n_targets >= 0 && d.n_targets <= PNPP_AUG_MAX_TARGETS, PNPP_ERR_ARG, "augment_clouds: n_targets=%d, at most %d per launch",
                 d.n_targets, PNPP_AUG_MAX_TARGETS);
    for (int t = 0; t < d.n_targets; ++t) {
        const pnpp_augment_target &g = d.targets[t];
        PNPP_REQUIRE(g.kind >= PNPP_AUG_ANGLE && g.kind <= PNPP_AUG_DIR8, PNPP_ERR_ARG, "augment_clouds: target %d has unknown kind %d", t,
                     g.kind);
        PNPP_REQUIRE(g.in && g.out && g.in != g.out, PNPP_ERR_ARG, "augment_clouds: target %d: null or aliased pointer", t);
        PNPP_REQUIRE(g.rows > 0, PNPP_ERR_ARG, "augment_clouds: target %d: rows=%d", t, g.rows);
        const bool cols_ok = g.kind == PNPP_AUG_ANGLE ? g.cols == 1 : g.kind == PNPP_AUG_VM ? (g.cols == 2 || g.cols == 3) : g.cols == 3;
        PNPP_REQUIRE(cols_ok, PNPP_ERR_ARG, "augment_clouds: target %d of kind %d cannot have %d columns", t, g.kind, g.cols);
        if (g.kind == PNPP_AUG_DIR8)
            PNPP_REQUIRE(g.rows == 1 && d.dirs8, PNPP_ERR_ARG, "augment_clouds: target %d: DIR8 takes one axis per cloud and needs dirs8", t);
    }
    const long long tiles = (N + kAugTile - 1) / kAugTile;
    const bool vec4 = (N * C) % 4 == 0 && ((uintptr_t)xyz_in % 16 == 0) && ((uintptr_t)xyz_out % 16 == 0);
    ProfScope ps(as_stream(stream), "augment_clouds_kernel B=%d N=%lld C=%d vec=%d targets=%d", B, (long long)N, C, vec4 ? 4 : 1, d.n_targets);
    const dim3 grid((unsigned)tiles, (unsigned)B);
    if (vec4)
        hipLaunchKernelGGL(augment_clouds_kernel<4>, grid, dim3(kAugTile), 0, as_stream(stream), (unsigned)seed, (unsigned)(seed >> 32),
                           (unsigned)stream_id, (unsigned)(stream_id >> 32), xyz_in, xyz_out, lengths, (long long)N, C, d, params_out);
    else
        hipLaunchKernelGGL(augment_clouds_kernel<1>, grid, dim3(kAugTile), 0, as_stream(stream), (unsigned)seed, (unsigned)(seed >> 32),
                           (unsigned)stream_id, (unsigned)(stream_id >> 32), xyz_in, xyz_out, lengths, (long long)N, C, d, params_out);
    PNPP_CHECK_LAUNCH("augment_clouds");
    return PNPP_OK;
}
