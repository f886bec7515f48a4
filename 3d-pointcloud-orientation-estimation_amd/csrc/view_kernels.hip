// view_kernels.hip -- single-view scan simulation of a device-resident batch for gfx950 (MI355X): per cloud one viewing direction, an
// orthographic depth buffer over the view plane, and the points the viewer cannot see removed -- survivors compacted in input order,
// the rest of the rows exact zeros, one launch, nothing read back.
//
// One workgroup of 1024 threads per cloud, three passes over its rows in global memory (a 10,000-point cloud is 120 KB: it stays in
// L2): (1) the extent of the projected cloud, (2) the depth buffer -- G x G words of LDS, one LDS atomicMax per point and splat cell,
// (3) the visibility test and a stable compaction: ballot + wave prefix + a cross-wave prefix in LDS, a running base carried from
// tile to tile.  No global atomics.
//
// Reproducibility: every float32 step is an IEEE basic operation in a fixed order (this file is compiled with -ffp-contract=off and
// spells the operations out); min, max and the depth buffer's max do not depend on the order they are taken in; the per-cloud angles
// are float64 rounded once.  tests/view_ref.py is the CPU restatement.
#include "common.h"
#include "sampler_device.h"

#pragma clang fp contract(off)

namespace pnpp {

constexpr int kViewTile = 1024;              // rows per compaction tile = threads per workgroup
constexpr int kViewWaves = kViewTile / 64;
constexpr double kViewTwoPiOver2p32 = 6.283185307179586476925286766559 / 4294967296.0;   // exact: a power-of-two division

struct ViewBasis {
    float vx, vy, vz;   // towards the viewer
    float rx, rz;       // r = (rx, 0, rz): the view plane's horizontal axis
    float ux, uy, uz;   // u: its vertical axis
    float azimuth, elevation;
    double ratio2p32;   // thinning: a visible point survives iff its word >= this (0: every word does)
};

// v = (ce sa, se, -ce ca), r = (ca, 0, sa), u = (-se sa, ce, se ca) from the float32 roundings of the four float64 values
__device__ __forceinline__ void view_basis_from(ViewBasis &q, double ca, double sa, double ce, double se) {
    const float fca = (float)ca, fsa = (float)sa, fce = (float)ce, fse = (float)se;
    q.vx = __fmul_rn(fce, fsa), q.vy = fse, q.vz = -__fmul_rn(fce, fca);
    q.rx = fca, q.rz = fsa;
    q.ux = -__fmul_rn(fse, fsa), q.uy = fce, q.uz = __fmul_rn(fse, fca);
}

__device__ __forceinline__ ViewBasis view_cloud_params(const pnpp_view_desc &d, unsigned b, unsigned str_lo, unsigned str_hi,
                                                       unsigned seed_lo, unsigned seed_hi) {
    ViewBasis q;
    q.ratio2p32 = 0.0;
    const bool given = (d.flags & (PNPP_VIEW_DIRS | PNPP_VIEW_ANGLES)) != 0;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (!given || d.drop > 0.0f) w = philox4(0xFFFFFFFFu, b, str_lo, str_hi, seed_lo, seed_hi);
    if (d.drop > 0.0f) q.ratio2p32 = (double)d.drop * (double)w.z;
    if (d.flags & PNPP_VIEW_DIRS) {
        const float *g = d.view_dirs + (size_t)b * 3;
        const double x = (double)g[0], y = (double)g[1], z = (double)g[2];
        const double len = sqrt(x * x + y * y + z * z);
        double ca = 1.0, sa = 0.0, ce = 1.0, se = 0.0;   // a zero or non-finite direction: azimuth 0, elevation 0
        if (len > 0.0 && len < (double)INFINITY) {
            const double nx = x / len, ny = y / len, nz = z / len;
            se = ny, ce = sqrt(nx * nx + nz * nz);
            if (ce > 0.0) sa = nx / ce, ca = -nz / ce;
        }
        view_basis_from(q, ca, sa, ce, se);
        q.azimuth = (float)atan2(sa, ca), q.elevation = (float)atan2(se, ce);
        return q;
    }
    double phi, eps;
    if (d.flags & PNPP_VIEW_ANGLES) {
        phi = (double)d.view_dirs[(size_t)b * 2], eps = (double)d.view_dirs[(size_t)b * 2 + 1];
    } else {
        const double lo = (double)d.elev_lo, hi = (double)d.elev_hi;
        phi = (double)w.x * kViewTwoPiOver2p32;
        eps = lo + (hi - lo) * ((double)w.y * (1.0 / 4294967296.0));
    }
    view_basis_from(q, cos(phi), sin(phi), cos(eps), sin(eps));
    q.azimuth = (float)phi, q.elevation = (float)eps;
    return q;
}

// p . e: three products, two sums, in x, y, z order
__device__ __forceinline__ float view_dot(float x, float y, float z, float ex, float ey, float ez) {
    return __fadd_rn(__fadd_rn(__fmul_rn(x, ex), __fmul_rn(y, ey)), __fmul_rn(z, ez));
}

// the order-preserving unsigned image of a float and back; 0 is below every image: the empty cell
__device__ __forceinline__ unsigned view_key(float d) {
    const unsigned u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float view_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// min(G - 1, floor((a - amin) / cell)), clamped in float so that no input (NaN, overflow) can index out of the grid
__device__ __forceinline__ int view_cell(float a, float amin, float cell, int G) {
    if (!(cell > 0.0f)) return 0;
    const float q = floorf(__fdiv_rn(__fsub_rn(a, amin), cell));
    return (int)fmaxf(0.0f, fminf(q, (float)(G - 1)));
}

template <bool IS_MIN>
__device__ __forceinline__ float view_wave_reduce(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        v = IS_MIN ? fminf(v, w) : fmaxf(v, w);
    }
    return v;
}

// grid (B), 1024 threads, dynamic LDS: G G words.  RAGGED: cloud b holds Nv = min(max(lengths_in[b], 1), N) rows.
template <bool RAGGED>
__global__ __launch_bounds__(kViewTile) void view_clouds_kernel(unsigned seed_lo, unsigned seed_hi, unsigned str_lo, unsigned str_hi,
                                                                const float *__restrict__ xyz_in, float *__restrict__ xyz_out,
                                                                const int32_t *__restrict__ lengths_in, int32_t *__restrict__ lengths_out,
                                                                int32_t *__restrict__ index_out, int N, int C, pnpp_view_desc d,
                                                                float *__restrict__ params) {
    extern __shared__ __attribute__((aligned(16))) unsigned zbuf[];   // G G depth words
    __shared__ float red[4][kViewWaves];
    __shared__ int wsum[2][kViewWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = d.G, splat = d.splat;
    int Nv = N;
    if constexpr (RAGGED) Nv = min(max(lengths_in[b], 1), N);
    const float *__restrict__ in = xyz_in + (size_t)b * (size_t)N * (size_t)C;
    float *__restrict__ out = xyz_out + (size_t)b * (size_t)N * (size_t)C;
    int32_t *__restrict__ idx = index_out ? index_out + (size_t)b * (size_t)N : nullptr;
    const ViewBasis q = view_cloud_params(d, (unsigned)b, str_lo, str_hi, seed_lo, seed_hi);

    for (int i = tid; i < G * G; i += kViewTile) zbuf[i] = 0u;

    // ---- pass 1: the extent of the projection
    float amin = INFINITY, amax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
    for (int n = tid; n < Nv; n += kViewTile) {
        const float *p = in + (size_t)n * C;
        const float x = p[0], y = p[1], z = p[2];
        const float a = view_dot(x, y, z, q.rx, 0.0f, q.rz), t = view_dot(x, y, z, q.ux, q.uy, q.uz);
        amin = fminf(amin, a), amax = fmaxf(amax, a), tmin = fminf(tmin, t), tmax = fmaxf(tmax, t);
    }
    amin = view_wave_reduce<true>(amin), amax = view_wave_reduce<false>(amax);
    tmin = view_wave_reduce<true>(tmin), tmax = view_wave_reduce<false>(tmax);
    if (lane == 0) red[0][wave] = amin, red[1][wave] = amax, red[2][wave] = tmin, red[3][wave] = tmax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kViewWaves; ++w) {
        amin = fminf(amin, red[0][w]), amax = fmaxf(amax, red[1][w]);
        tmin = fminf(tmin, red[2][w]), tmax = fmaxf(tmax, red[3][w]);
    }
    // + 0: a zero of either sign becomes +0, so the bits do not depend on which of two equal zeros a min or max returned
    amin = __fadd_rn(amin, 0.0f), amax = __fadd_rn(amax, 0.0f), tmin = __fadd_rn(tmin, 0.0f), tmax = __fadd_rn(tmax, 0.0f);
    const float ext = fmaxf(__fsub_rn(amax, amin), __fsub_rn(tmax, tmin));
    const float cell = __fdiv_rn(ext, (float)G);
    const float thr = __fmul_rn(d.thickness, ext);

    // ---- pass 2: the depth buffer
    for (int n = tid; n < Nv; n += kViewTile) {
        const float *p = in + (size_t)n * C;
        const float x = p[0], y = p[1], z = p[2];
        const unsigned key = view_key(view_dot(x, y, z, q.vx, q.vy, q.vz));
        const int ia = view_cell(view_dot(x, y, z, q.rx, 0.0f, q.rz), amin, cell, G);
        const int it = view_cell(view_dot(x, y, z, q.ux, q.uy, q.uz), tmin, cell, G);
        for (int i = max(ia - splat, 0); i <= min(ia + splat, G - 1); ++i)
            for (int j = max(it - splat, 0); j <= min(it + splat, G - 1); ++j) atomicMax(&zbuf[i * G + j], key);
    }
    __syncthreads();

    // ---- pass 3: the test, the thinning and the stable compaction
    int kept = 0;   // survivors of the tiles so far: the same value in every thread
    for (int n0 = 0, par = 0; n0 < Nv; n0 += kViewTile, par ^= 1) {
        const int n = n0 + tid;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        bool keep = false;
        if (n < Nv) {
            const float *p = in + (size_t)n * C;
            x = p[0], y = p[1], z = p[2];
            const float dep = view_dot(x, y, z, q.vx, q.vy, q.vz);
            const int ia = view_cell(view_dot(x, y, z, q.rx, 0.0f, q.rz), amin, cell, G);
            const int it = view_cell(view_dot(x, y, z, q.ux, q.uy, q.uz), tmin, cell, G);
            keep = __fsub_rn(view_unkey(zbuf[ia * G + it]), dep) <= thr;
            if (keep && d.drop > 0.0f)
                keep = (double)philox4((unsigned)n, (unsigned)b, str_lo, str_hi, seed_lo, seed_hi).x >= q.ratio2p32;
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) wsum[par][wave] = __popcll(vote);
        __syncthreads();   // one barrier per tile: the next tile writes the other half of wsum
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kViewWaves; ++w) {
            const int c = wsum[par][w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (keep) {
            const int row = kept + before + __popcll(vote & ((1ull << lane) - 1ull));   // < Nv: one row per survivor, in order
            float *o = out + (size_t)row * C;
            o[0] = x, o[1] = y, o[2] = z;
            if (C == 6) {
                const float *p = in + (size_t)n * C;
                o[3] = p[3], o[4] = p[4], o[5] = p[5];
            }
            if (idx) idx[row] = n;
        }
        kept += total;
    }

    // ---- the floor: too few survivors, the cloud passes through whole
    const bool passed = kept < d.min_keep;
    if (passed) {
        __syncthreads();   // the survivors' rows are written again
        for (int i = tid; i < Nv * C; i += kViewTile) out[i] = in[i];
        if (idx)
            for (int n = tid; n < Nv; n += kViewTile) idx[n] = n;
        kept = Nv;
    }
    for (size_t i = (size_t)kept * C + tid; i < (size_t)N * C; i += kViewTile) out[i] = 0.0f;
    if (idx)
        for (int n = kept + tid; n < N; n += kViewTile) idx[n] = -1;
    if (tid == 0) {
        lengths_out[b] = kept;
        float *o = params + (size_t)b * 8;
        o[0] = q.vx, o[1] = q.vy, o[2] = q.vz, o[3] = q.azimuth, o[4] = q.elevation, o[5] = cell, o[6] = (float)kept;
        o[7] = passed ? 1.0f : 0.0f;
    }
}

}  // namespace pnpp

using namespace pnpp;

extern "C" int pnpp_view_clouds(uint64_t seed, uint64_t stream_id, const float *xyz_in, float *xyz_out, const int32_t *lengths_in,
                                int32_t *lengths_out, int32_t *index_out, int B, int64_t N, int C, const pnpp_view_desc *desc,
                                float *params_out, void *stream) {
    PNPP_REQUIRE(xyz_in && xyz_out && lengths_out && desc && params_out, PNPP_ERR_ARG, "view_clouds: null pointer");
    PNPP_REQUIRE(xyz_in != xyz_out, PNPP_ERR_ARG, "view_clouds: out of place only (xyz_in == xyz_out)");
    PNPP_REQUIRE(C == 3 || C == 6, PNPP_ERR_ARG, "view_clouds: C=%d: rows are xyz (3) or xyz + normal (6)", C);
    PNPP_REQUIRE(B > 0 && B <= 65535, PNPP_ERR_ARG, "view_clouds: B=%d must be 1..65535", B);
    PNPP_REQUIRE(N > 0 && N <= (1ll << 24), PNPP_ERR_ARG, "view_clouds: N=%lld must be 1..2^24 (the survivor count is kept in a float32)",
                 (long long)N);
    const pnpp_view_desc &d = *desc;
    PNPP_REQUIRE(d.G >= 1 && d.G <= PNPP_VIEW_MAX_G, PNPP_ERR_ARG, "view_clouds: G=%d: the depth buffer is 1..%d cells a side", d.G,
                 PNPP_VIEW_MAX_G);
    PNPP_REQUIRE(d.splat >= 0 && d.splat <= 2, PNPP_ERR_ARG, "view_clouds: splat=%d must be 0..2", d.splat);
    PNPP_REQUIRE(d.thickness >= 0.0f && d.thickness < INFINITY, PNPP_ERR_ARG, "view_clouds: thickness=%g must be finite and >= 0",
                 (double)d.thickness);
    const float half_pi = 1.57079637f;   // float32(pi / 2)
    PNPP_REQUIRE(d.elev_lo >= -half_pi && d.elev_hi <= half_pi && d.elev_lo <= d.elev_hi, PNPP_ERR_ARG,
                 "view_clouds: elevation range must satisfy -pi/2 <= lo <= hi <= pi/2 (lo=%g hi=%g)", (double)d.elev_lo, (double)d.elev_hi);
    PNPP_REQUIRE(d.drop >= 0.0f && d.drop < 1.0f, PNPP_ERR_ARG, "view_clouds: drop=%g must be in [0, 1)", (double)d.drop);
    PNPP_REQUIRE(d.min_keep >= 0 && (long long)d.min_keep <= (long long)N, PNPP_ERR_ARG, "view_clouds: min_keep=%d must be 0..N=%lld",
                 d.min_keep, (long long)N);
    PNPP_REQUIRE(!(d.flags & ~(PNPP_VIEW_DIRS | PNPP_VIEW_ANGLES)), PNPP_ERR_ARG, "view_clouds: unknown flag bits 0x%x", d.flags);
    PNPP_REQUIRE((d.flags & (PNPP_VIEW_DIRS | PNPP_VIEW_ANGLES)) != (PNPP_VIEW_DIRS | PNPP_VIEW_ANGLES), PNPP_ERR_ARG,
                 "view_clouds: view_dirs holds directions or angles, not both (flags 0x%x)", d.flags);
    PNPP_REQUIRE((d.view_dirs != nullptr) == ((d.flags & (PNPP_VIEW_DIRS | PNPP_VIEW_ANGLES)) != 0), PNPP_ERR_ARG,
                 "view_clouds: view_dirs and its flag (PNPP_VIEW_DIRS or PNPP_VIEW_ANGLES) go together");
    const size_t lds = (size_t)d.G * d.G * sizeof(unsigned);
    const auto kfn = lengths_in ? view_clouds_kernel<true> : view_clouds_kernel<false>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    ProfScope ps(as_stream(stream), "view_clouds_kernel B=%d N=%lld C=%d G=%d splat=%d ragged=%d", B, (long long)N, C, d.G, d.splat,
                 lengths_in ? 1 : 0);
    hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(kViewTile), lds, as_stream(stream), (unsigned)seed, (unsigned)(seed >> 32),
                       (unsigned)stream_id, (unsigned)(stream_id >> 32), xyz_in, xyz_out, lengths_in, lengths_out, index_out, (int)N, C, d,
                       params_out);
    PNPP_CHECK_LAUNCH("view_clouds");
    return PNPP_OK;
}
