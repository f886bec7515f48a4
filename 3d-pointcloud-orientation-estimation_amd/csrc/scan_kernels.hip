// scan_kernels.hip -- raw-scan preparation of a device-resident ragged batch for gfx950 (MI355X): a voxel-grid downsample that keeps
// one real point per occupied cell, statistical outlier removal over given neighbour lists, and the unit frame (centre and scale).
// Every step has pnpp_view_clouds' contract: ragged in, ragged out, survivors in input order, exact zeros behind them, lengths' and
// optionally the source rows, nothing read back, capturable, two calls bit-identical.
//
// Voxel grid: four launches.  (1) clear: the per-cloud open-addressing table (32-bit cell ids, 64-bit winners) and the six bound
// words; (2) bounds: several workgroups per cloud, wave reductions, one integer atomicMin / atomicMax per wave and axis on the
// order-preserving image of the float; (3) insert: several workgroups per cloud, a compare-and-swap claims the cell's slot (linear
// probing), an unsigned 64-bit atomicMin of (bits(d) << 32 | row) takes the winner -- d >= 0, so its bits order as d does, and the
// winner of a cell depends neither on the slot it landed in nor on the order of arrival; (4) compact: one workgroup per cloud, a row
// survives when the table holds its own key, then ballot + wave prefix + cross-wave prefix + a running base.  The table is global
// memory (2 N .. 4 N slots, 12 bytes each) so that the insert phase is not held to one workgroup's LDS.  No floating-point atomics.
//
// Outliers: a thread per point sums sqrt((double) d) over its list in list order; one workgroup per cloud reduces mean and population
// standard deviation in float64 in a fixed order (per-thread strided partials, wave butterfly, waves in order), thresholds, compacts.
//
// Reproducibility: every float32 step is an IEEE basic operation in a fixed order (this file is compiled with -ffp-contract=off and
// spells the operations out); min and max do not depend on the order they are taken in.  tests/scan_ref.py is the CPU restatement.
#include "common.h"

#pragma clang fp contract(off)

#include "exact_dist.h"

namespace pnpp {

constexpr int kScanTile = 1024;                 // rows per compaction tile = threads of a per-cloud workgroup
constexpr int kScanWaves = kScanTile / 64;
constexpr int kScanWide = 256;                  // threads of a workgroup of the phases that take several per cloud
constexpr int kScanRowsPerBlock = 4096;         // rows such a workgroup walks
constexpr int kScanMaxBlocks = 64;              // per cloud
constexpr unsigned kVoxEmpty = 0xFFFFFFFFu;     // cell ids are 30 bits
constexpr unsigned long long kVoxNone = ~0ull;
constexpr size_t kVoxMinSlots = 64;

__device__ __forceinline__ float scan_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ __forceinline__ int scan_valid_rows(const int32_t *lengths, int b, int N) { return lengths ? min(max(lengths[b], 1), N) : N; }

template <bool IS_MIN>
__device__ __forceinline__ float scan_wave_reduce(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        v = IS_MIN ? fminf(v, w) : fmaxf(v, w);
    }
    return v;
}

// the sum of one double per thread of a 1024-thread workgroup, the same bits in every thread: butterfly over the lanes (every lane ends
// with the same association), then the sixteen waves in wave order.  One barrier after the write; `slab` is free again after the next.
__device__ __forceinline__ double scan_block_sum(double v, double *slab) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += shfl_xor_f64(v, o);
    if ((threadIdx.x & 63) == 0) slab[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) s += slab[w];
    return s;
}

// Stable compaction by one 1024-thread workgroup: rows n < Nv with keep(n) go to rows 0 .. kept-1 of `out` in their order (C == 6:
// columns 3..5 travel untouched), rows kept .. N-1 become exact zeros, idx (optional) the source row and -1.  Returns kept, the same
// value in every thread.  wsum: 2 x kScanWaves ints of LDS, one barrier per tile.
template <typename Keep>
__device__ __forceinline__ int scan_compact(const float *__restrict__ in, float *__restrict__ out, int32_t *__restrict__ idx, int Nv, int N,
                                            int C, int (*wsum)[kScanWaves], Keep keep_row) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int kept = 0;
    for (int n0 = 0, par = 0; n0 < Nv; n0 += kScanTile, par ^= 1) {
        const int n = n0 + tid;
        const bool keep = n < Nv && keep_row(n);
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) wsum[par][wave] = __popcll(vote);
        __syncthreads();   // the next tile writes the other half of wsum
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) {
            const int c = wsum[par][w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (keep) {
            const int row = kept + before + __popcll(vote & ((1ull << lane) - 1ull));   // <= n < Nv
            const float *p = in + (size_t)n * C;
            float *o = out + (size_t)row * C;
            for (int c = 0; c < C; ++c) o[c] = p[c];
            if (idx) idx[row] = n;
        }
        kept += total;
    }
    for (size_t i = (size_t)kept * C + tid; i < (size_t)N * C; i += kScanTile) out[i] = 0.0f;
    if (idx)
        for (int n = kept + tid; n < N; n += kScanTile) idx[n] = -1;
    return kept;
}

// ---- voxel grid --------------------------------------------------------------------------------------------------------------------
struct VoxelWs {
    unsigned *bounds;            // (B, 8): images of lo x y z, hi x y z, two unused
    unsigned *keys;              // (B, slots)
    unsigned long long *vals;    // (B, slots)
    size_t slots;                // a power of two, >= 2 N
    int shift;                   // 32 - log2(slots)
};

struct VoxelFrame {
    float lo[3], hi[3], h;
    float cmax;   // the last cell index per axis: grid - 1 (the cloud's far face belongs to the last cell), or 1023
};

// lo, hi (a zero of either sign taken as +0) and the cell edge: `cell`, or with grid > 0 the longest extent over grid (0: 1)
__device__ __forceinline__ VoxelFrame voxel_frame(const unsigned *bw, float cell, int grid) {
    VoxelFrame f;
#pragma unroll
    for (int a = 0; a < 3; ++a) f.lo[a] = __fadd_rn(scan_unkey(bw[a]), 0.0f), f.hi[a] = __fadd_rn(scan_unkey(bw[3 + a]), 0.0f);
    f.h = cell;
    f.cmax = grid > 0 ? (float)(grid - 1) : 1023.0f;
    if (grid > 0) {
        const float ext = fmaxf(fmaxf(__fsub_rn(f.hi[0], f.lo[0]), __fsub_rn(f.hi[1], f.lo[1])), __fsub_rn(f.hi[2], f.lo[2]));
        f.h = __fdiv_rn(ext, (float)grid);
    }
    if (!(f.h > 0.0f)) f.h = 1.0f;
    return f;
}

// the 30-bit cell id of a point and its 64-bit key: the cell index is clamped in float, so no input can leave the ten bits
__device__ __forceinline__ void voxel_cell_key(const VoxelFrame &f, float x, float y, float z, unsigned row, unsigned &id,
                                               unsigned long long &key) {
    const float p[3] = {x, y, z};
    float m[3];
    id = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = floorf(__fdiv_rn(__fsub_rn(p[a], f.lo[a]), f.h));
        const float c = fmaxf(0.0f, fminf(q, f.cmax));
        id |= (unsigned)(int)c << (10 * a);
        m[a] = __fadd_rn(f.lo[a], __fmul_rn(__fadd_rn(c, 0.5f), f.h));
    }
    const float d = direct_dist_exact(x, y, z, m[0], m[1], m[2]);
    key = ((unsigned long long)__float_as_uint(d) << 32) | row;
}

__device__ __forceinline__ unsigned voxel_hash(unsigned id, int shift) { return (id * 0x9E3779B1u) >> shift; }

// grid-stride fill of the whole workspace: keys empty, winners none, lower bounds above and upper bounds below every image
__global__ __launch_bounds__(kScanWide) void voxel_clear_kernel(VoxelWs W, size_t total_slots, int B) {
    const size_t stride = (size_t)gridDim.x * kScanWide;
    for (size_t i = (size_t)blockIdx.x * kScanWide + threadIdx.x; i < total_slots; i += stride) W.keys[i] = kVoxEmpty, W.vals[i] = kVoxNone;
    for (size_t i = (size_t)blockIdx.x * kScanWide + threadIdx.x; i < (size_t)B * 8; i += stride) W.bounds[i] = (i & 7) < 3 ? 0xFFFFFFFFu : 0u;
}

// grid (blocks, B), 256 threads
__global__ __launch_bounds__(kScanWide) void voxel_bounds_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ lengths,
                                                                 int N, int C, VoxelWs W) {
    const int b = blockIdx.y, Nv = scan_valid_rows(lengths, b, N);
    const float *__restrict__ in = xyz + (size_t)b * (size_t)N * (size_t)C;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int n = blockIdx.x * kScanWide + threadIdx.x; n < Nv; n += gridDim.x * kScanWide) {
        const float *p = in + (size_t)n * C;
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], p[a]), hi[a] = fmaxf(hi[a], p[a]);
    }
    if (blockIdx.x * kScanWide + (threadIdx.x & ~63) >= Nv) return;   // the wave saw no row (wave-uniform)
    unsigned *bw = W.bounds + (size_t)b * 8;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = scan_wave_reduce<true>(lo[a]), h = scan_wave_reduce<false>(hi[a]);
        if ((threadIdx.x & 63) == 0) atomicMin(bw + a, f32_sortable(l)), atomicMax(bw + 3 + a, f32_sortable(h));
    }
}

// grid (blocks, B), 256 threads: every valid row claims its cell's slot and offers its key
__global__ __launch_bounds__(kScanWide) void voxel_insert_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ lengths,
                                                                 int N, int C, float cell, int grid, VoxelWs W) {
    const int b = blockIdx.y, Nv = scan_valid_rows(lengths, b, N);
    const float *__restrict__ in = xyz + (size_t)b * (size_t)N * (size_t)C;
    const VoxelFrame f = voxel_frame(W.bounds + (size_t)b * 8, cell, grid);
    unsigned *keys = W.keys + (size_t)b * W.slots;
    unsigned long long *vals = W.vals + (size_t)b * W.slots;
    const unsigned mask = (unsigned)(W.slots - 1);
    for (int n = blockIdx.x * kScanWide + threadIdx.x; n < Nv; n += gridDim.x * kScanWide) {
        const float *p = in + (size_t)n * C;
        unsigned id;
        unsigned long long key;
        voxel_cell_key(f, p[0], p[1], p[2], (unsigned)n, id, key);
        unsigned slot = voxel_hash(id, W.shift);
        for (size_t probe = 0; probe < W.slots; ++probe, slot = (slot + 1) & mask) {   // at most Nv <= slots / 2 cells: an end exists
            const unsigned prev = atomicCAS(keys + slot, kVoxEmpty, id);
            if (prev == kVoxEmpty || prev == id) {
                atomicMin(vals + slot, key);
                break;
            }
        }
    }
}

// grid (B), 1024 threads
__global__ __launch_bounds__(kScanTile) void voxel_compact_kernel(const float *__restrict__ xyz_in, float *__restrict__ xyz_out,
                                                                  const int32_t *__restrict__ lengths_in, int32_t *__restrict__ lengths_out,
                                                                  int32_t *__restrict__ index_out, int N, int C, float cell, int grid,
                                                                  VoxelWs W) {
    __shared__ int wsum[2][kScanWaves];
    const int b = blockIdx.x, Nv = scan_valid_rows(lengths_in, b, N);
    const float *__restrict__ in = xyz_in + (size_t)b * (size_t)N * (size_t)C;
    const VoxelFrame f = voxel_frame(W.bounds + (size_t)b * 8, cell, grid);
    const unsigned *keys = W.keys + (size_t)b * W.slots;
    const unsigned long long *vals = W.vals + (size_t)b * W.slots;
    const unsigned mask = (unsigned)(W.slots - 1);
    const int kept = scan_compact(in, xyz_out + (size_t)b * (size_t)N * (size_t)C, index_out ? index_out + (size_t)b * (size_t)N : nullptr,
                                  Nv, N, C, wsum, [&](int n) {
                                      const float *p = in + (size_t)n * C;
                                      unsigned id;
                                      unsigned long long key;
                                      voxel_cell_key(f, p[0], p[1], p[2], (unsigned)n, id, key);
                                      unsigned slot = voxel_hash(id, W.shift);
                                      for (size_t probe = 0; probe < W.slots; ++probe, slot = (slot + 1) & mask) {
                                          const unsigned k = keys[slot];
                                          if (k == id) return vals[slot] == key;
                                          if (k == kVoxEmpty) return false;   // cannot happen: the row was inserted
                                      }
                                      return false;
                                  });
    if (threadIdx.x == 0) lengths_out[b] = kept;
}

// ---- statistical outliers ----------------------------------------------------------------------------------------------------------
// grid (cdiv(N, 256), B), 256 threads: s[b, n] = (sum over the k + 1 list entries of sqrt((double) d)) / k, 0 in the padding
__global__ __launch_bounds__(kScanWide) void outlier_statistic_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ lists,
                                                                      const int32_t *__restrict__ lengths, int N, int C, int k,
                                                                      double *__restrict__ stat) {
    const int b = blockIdx.y, n = blockIdx.x * kScanWide + threadIdx.x, Nv = scan_valid_rows(lengths, b, N);
    if (n >= N) return;
    double s = 0.0;
    if (n < Nv) {
        const float *__restrict__ in = xyz + (size_t)b * (size_t)N * (size_t)C;
        const int32_t *list = lists + ((size_t)b * (size_t)N + n) * (size_t)(k + 1);
        const float *p = in + (size_t)n * C;
        const float x = p[0], y = p[1], z = p[2];
        for (int j = 0; j <= k; ++j) {
            const int m = min(max(list[j], 0), Nv - 1);   // a list of the search is already inside; a given one cannot leave the cloud
            const float *q = in + (size_t)m * C;
            s += __dsqrt_rn((double)direct_dist_exact(x, y, z, q[0], q[1], q[2]));
        }
        s = s / (double)k;
    }
    stat[(size_t)b * (size_t)N + n] = s;
}

// grid (B), 1024 threads: mean, population standard deviation, threshold, compaction.  Nv <= k: the cloud passes through whole.
__global__ __launch_bounds__(kScanTile) void outlier_filter_kernel(const float *__restrict__ xyz_in, float *__restrict__ xyz_out,
                                                                   const double *__restrict__ stat, const int32_t *__restrict__ lengths_in,
                                                                   int32_t *__restrict__ lengths_out, int32_t *__restrict__ index_out,
                                                                   double *__restrict__ stats_out, int N, int C, int k, double std_ratio) {
    __shared__ int wsum[2][kScanWaves];
    __shared__ double slab[2][kScanWaves];
    const int b = blockIdx.x, tid = threadIdx.x, Nv = scan_valid_rows(lengths_in, b, N);
    const double *__restrict__ s = stat + (size_t)b * (size_t)N;
    const bool whole = Nv <= k;
    double mean = 0.0, sd = 0.0, thr = (double)INFINITY;
    if (!whole) {   // uniform over the workgroup
        double acc = 0.0;
        for (int n = tid; n < Nv; n += kScanTile) acc += s[n];
        mean = scan_block_sum(acc, slab[0]) / (double)Nv;
        acc = 0.0;
        for (int n = tid; n < Nv; n += kScanTile) {
            const double d = s[n] - mean;
            acc += d * d;
        }
        sd = __dsqrt_rn(scan_block_sum(acc, slab[1]) / (double)Nv);
        thr = mean + std_ratio * sd;
    }
    const int kept = scan_compact(xyz_in + (size_t)b * (size_t)N * (size_t)C, xyz_out + (size_t)b * (size_t)N * (size_t)C,
                                  index_out ? index_out + (size_t)b * (size_t)N : nullptr, Nv, N, C, wsum,
                                  [&](int n) { return whole || s[n] <= thr; });
    if (tid == 0) {
        lengths_out[b] = kept;
        if (stats_out) {
            double *o = stats_out + (size_t)b * 4;
            o[0] = mean, o[1] = sd, o[2] = thr, o[3] = (double)kept;
        }
    }
}

// ---- unit frame --------------------------------------------------------------------------------------------------------------------
// grid (B), 1024 threads.  centre_mode / scale_mode: PNPP_SCAN_NONE, _CENTROID | _SPHERE, _BOX.
__global__ __launch_bounds__(kScanTile) void normalize_clouds_kernel(const float *__restrict__ xyz_in, float *__restrict__ xyz_out,
                                                                     const int32_t *__restrict__ lengths, int N, int C, int centre_mode,
                                                                     int scale_mode, float *__restrict__ centre_out,
                                                                     float *__restrict__ scale_out) {
    __shared__ double slab[3][kScanWaves];
    __shared__ float red[7][kScanWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Nv = scan_valid_rows(lengths, b, N);
    const float *__restrict__ in = xyz_in + (size_t)b * (size_t)N * (size_t)C;
    float *__restrict__ out = xyz_out + (size_t)b * (size_t)N * (size_t)C;
    float c[3] = {0.0f, 0.0f, 0.0f}, r = 1.0f;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (centre_mode == PNPP_SCAN_BOX || scale_mode == PNPP_SCAN_BOX) {
        for (int n = tid; n < Nv; n += kScanTile) {
            const float *p = in + (size_t)n * C;
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], p[a]), hi[a] = fmaxf(hi[a], p[a]);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = scan_wave_reduce<true>(lo[a]), hi[a] = scan_wave_reduce<false>(hi[a]);
            if (lane == 0) red[a][wave] = lo[a], red[3 + a][wave] = hi[a];
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            for (int w = 0; w < kScanWaves; ++w) lo[a] = fminf(lo[a], red[a][w]), hi[a] = fmaxf(hi[a], red[3 + a][w]);
            lo[a] = __fadd_rn(lo[a], 0.0f), hi[a] = __fadd_rn(hi[a], 0.0f);   // a zero of either sign becomes +0
        }
    }
    if (centre_mode == PNPP_SCAN_CENTROID) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int n = tid; n < Nv; n += kScanTile) {
            const float *p = in + (size_t)n * C;
            acc[0] += (double)p[0], acc[1] += (double)p[1], acc[2] += (double)p[2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = (float)(scan_block_sum(acc[a], slab[a]) / (double)Nv);
    } else if (centre_mode == PNPP_SCAN_BOX) {
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = __fmul_rn(0.5f, __fadd_rn(lo[a], hi[a]));
    }
    if (scale_mode == PNPP_SCAN_SPHERE) {
        float m = 0.0f;
        for (int n = tid; n < Nv; n += kScanTile) {
            const float *p = in + (size_t)n * C;
            m = fmaxf(m, sq3_exact(__fsub_rn(p[0], c[0]), __fsub_rn(p[1], c[1]), __fsub_rn(p[2], c[2])));
        }
        m = scan_wave_reduce<false>(m);
        if (lane == 0) red[6][wave] = m;
        __syncthreads();
        for (int w = 0; w < kScanWaves; ++w) m = fmaxf(m, red[6][w]);
        r = sqrtf(m);   // correctly rounded (hipcc's default for float32 sqrt and divide); __fsqrt_rn is the native approximation here
    } else if (scale_mode == PNPP_SCAN_BOX) {
        r = __fmul_rn(0.5f, fmaxf(fmaxf(__fsub_rn(hi[0], lo[0]), __fsub_rn(hi[1], lo[1])), __fsub_rn(hi[2], lo[2])));
    }
    if (!(r > 0.0f)) r = 1.0f;
    for (int n = tid; n < Nv; n += kScanTile) {
        const float *p = in + (size_t)n * C;
        float *o = out + (size_t)n * C;
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = __fdiv_rn(__fsub_rn(p[a], c[a]), r);
        for (int a = 3; a < C; ++a) o[a] = p[a];
    }
    for (size_t i = (size_t)Nv * C + tid; i < (size_t)N * C; i += kScanTile) out[i] = 0.0f;
    if (tid < 3) centre_out[(size_t)b * 3 + tid] = c[tid];
    if (tid == 0) scale_out[b] = r;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static size_t voxel_slots(int64_t N) {
    size_t s = kVoxMinSlots;
    while (s < 2 * (size_t)N) s <<= 1;
    return s;
}

static VoxelWs voxel_carve(void *workspace, int B, int64_t N, size_t *bytes) {
    VoxelWs W;
    W.slots = voxel_slots(N);
    W.shift = 32;
    for (size_t s = W.slots; s > 1; s >>= 1) --W.shift;
    Carver cv(workspace);
    W.bounds = cv.take<unsigned>((size_t)B * 8);
    W.keys = cv.take<unsigned>((size_t)B * W.slots);
    W.vals = cv.take<unsigned long long>((size_t)B * W.slots);
    *bytes = cv.bytes();
    return W;
}

static bool scan_shape_ok(const char *what, int B, int64_t N, int C) {
    PNPP_REQUIRE(C == 3 || C == 6, false, "%s: C=%d: rows are xyz (3) or xyz + normal (6)", what, C);
    PNPP_REQUIRE(B > 0 && B <= 65535, false, "%s: B=%d must be 1..65535", what, B);
    PNPP_REQUIRE(N > 0 && N <= (1ll << 24), false, "%s: N=%lld must be 1..2^24", what, (long long)N);
    return true;
}

static unsigned scan_blocks(int64_t N) {
    const int64_t g = (N + kScanRowsPerBlock - 1) / kScanRowsPerBlock;
    return (unsigned)(g < 1 ? 1 : (g > kScanMaxBlocks ? kScanMaxBlocks : g));
}

}  // namespace pnpp

using namespace pnpp;

extern "C" size_t pnpp_voxel_workspace_bytes(int B, int64_t N) {
    if (!scan_shape_ok("voxel_workspace_bytes", B, N, 3)) return 0;
    size_t bytes = 0;
    (void)voxel_carve(nullptr, B, N, &bytes);
    return bytes;
}

extern "C" int pnpp_voxel_downsample(const float *xyz_in, float *xyz_out, const int32_t *lengths_in, int32_t *lengths_out,
                                     int32_t *index_out, int B, int64_t N, int C, float cell, int grid, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    PNPP_REQUIRE(xyz_in && xyz_out && lengths_out && workspace, PNPP_ERR_ARG, "voxel_downsample: null pointer");
    PNPP_REQUIRE(xyz_in != xyz_out, PNPP_ERR_ARG, "voxel_downsample: out of place only (xyz_in == xyz_out)");
    if (!scan_shape_ok("voxel_downsample", B, N, C)) return PNPP_ERR_ARG;
    PNPP_REQUIRE((grid == 0) != !(cell > 0.0f && cell < INFINITY), PNPP_ERR_ARG,
                 "voxel_downsample: exactly one of cell (finite, > 0) and grid (1..%d) is given, got cell=%g grid=%d", PNPP_VOXEL_MAX_GRID,
                 (double)cell, grid);
    PNPP_REQUIRE(grid >= 0 && grid <= PNPP_VOXEL_MAX_GRID, PNPP_ERR_ARG, "voxel_downsample: grid=%d must be 1..%d", grid, PNPP_VOXEL_MAX_GRID);
    size_t need = 0;
    const VoxelWs W = voxel_carve(workspace, B, N, &need);
    PNPP_REQUIRE(workspace_bytes >= need, PNPP_ERR_ARG, "voxel_downsample: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const hipStream_t st = as_stream(stream);
    const unsigned blocks = scan_blocks(N);
    const size_t total = (size_t)B * W.slots;
    const size_t clear_blocks = (total + kScanWide * 16 - 1) / (kScanWide * 16);
    {
        ProfScope ps(st, "voxel_clear_kernel B=%d slots=%zu", B, W.slots);
        hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)(clear_blocks > 4096 ? 4096 : clear_blocks)), dim3(kScanWide), 0, st, W, total, B);
        PNPP_CHECK_LAUNCH("voxel_downsample (clear)");
    }
    {
        ProfScope ps(st, "voxel_bounds_kernel B=%d N=%lld C=%d", B, (long long)N, C);
        hipLaunchKernelGGL(voxel_bounds_kernel, dim3(blocks, (unsigned)B), dim3(kScanWide), 0, st, xyz_in, lengths_in, (int)N, C, W);
        PNPP_CHECK_LAUNCH("voxel_downsample (bounds)");
    }
    {
        ProfScope ps(st, "voxel_insert_kernel B=%d N=%lld C=%d grid=%d", B, (long long)N, C, grid);
        hipLaunchKernelGGL(voxel_insert_kernel, dim3(blocks, (unsigned)B), dim3(kScanWide), 0, st, xyz_in, lengths_in, (int)N, C, cell, grid, W);
        PNPP_CHECK_LAUNCH("voxel_downsample (insert)");
    }
    {
        ProfScope ps(st, "voxel_compact_kernel B=%d N=%lld C=%d grid=%d", B, (long long)N, C, grid);
        hipLaunchKernelGGL(voxel_compact_kernel, dim3((unsigned)B), dim3(kScanTile), 0, st, xyz_in, xyz_out, lengths_in, lengths_out, index_out,
                           (int)N, C, cell, grid, W);
        PNPP_CHECK_LAUNCH("voxel_downsample (compact)");
    }
    return PNPP_OK;
}

extern "C" int pnpp_outlier_statistic(const float *xyz, const int32_t *lists, const int32_t *lengths, int B, int64_t N, int C, int k,
                                      double *statistic, void *stream) {
    PNPP_REQUIRE(xyz && lists && statistic, PNPP_ERR_ARG, "outlier_statistic: null pointer");
    if (!scan_shape_ok("outlier_statistic", B, N, C)) return PNPP_ERR_ARG;
    PNPP_REQUIRE(k >= 1 && k <= PNPP_OUTLIER_MAX_K, PNPP_ERR_ARG, "outlier_statistic: k=%d must be 1..%d", k, PNPP_OUTLIER_MAX_K);
    ProfScope ps(as_stream(stream), "outlier_statistic_kernel B=%d N=%lld C=%d k=%d", B, (long long)N, C, k);
    hipLaunchKernelGGL(outlier_statistic_kernel, dim3((unsigned)((N + kScanWide - 1) / kScanWide), (unsigned)B), dim3(kScanWide), 0,
                       as_stream(stream), xyz, lists, lengths, (int)N, C, k, statistic);
    PNPP_CHECK_LAUNCH("outlier_statistic");
    return PNPP_OK;
}

extern "C" int pnpp_outlier_filter(const float *xyz_in, float *xyz_out, const double *statistic, const int32_t *lengths_in,
                                   int32_t *lengths_out, int32_t *index_out, double *stats_out, int B, int64_t N, int C, int k,
                                   double std_ratio, void *stream) {
    PNPP_REQUIRE(xyz_in && xyz_out && statistic && lengths_out, PNPP_ERR_ARG, "outlier_filter: null pointer");
    PNPP_REQUIRE(xyz_in != xyz_out, PNPP_ERR_ARG, "outlier_filter: out of place only (xyz_in == xyz_out)");
    if (!scan_shape_ok("outlier_filter", B, N, C)) return PNPP_ERR_ARG;
    PNPP_REQUIRE(k >= 1 && k <= PNPP_OUTLIER_MAX_K, PNPP_ERR_ARG, "outlier_filter: k=%d must be 1..%d", k, PNPP_OUTLIER_MAX_K);
    PNPP_REQUIRE(std_ratio >= 0.0 && std_ratio < (double)INFINITY, PNPP_ERR_ARG, "outlier_filter: std_ratio=%g must be finite and >= 0",
                 std_ratio);
    ProfScope ps(as_stream(stream), "outlier_filter_kernel B=%d N=%lld C=%d k=%d", B, (long long)N, C, k);
    hipLaunchKernelGGL(outlier_filter_kernel, dim3((unsigned)B), dim3(kScanTile), 0, as_stream(stream), xyz_in, xyz_out, statistic, lengths_in,
                       lengths_out, index_out, stats_out, (int)N, C, k, std_ratio);
    PNPP_CHECK_LAUNCH("outlier_filter");
    return PNPP_OK;
}

extern "C" int pnpp_normalize_clouds(const float *xyz_in, float *xyz_out, const int32_t *lengths, int B, int64_t N, int C, int centre_mode,
                                     int scale_mode, float *centre_out, float *scale_out, void *stream) {
    PNPP_REQUIRE(xyz_in && xyz_out && centre_out && scale_out, PNPP_ERR_ARG, "normalize_clouds: null pointer");
    PNPP_REQUIRE(xyz_in != xyz_out, PNPP_ERR_ARG, "normalize_clouds: out of place only (xyz_in == xyz_out)");
    if (!scan_shape_ok("normalize_clouds", B, N, C)) return PNPP_ERR_ARG;
    PNPP_REQUIRE(centre_mode == PNPP_SCAN_NONE || centre_mode == PNPP_SCAN_CENTROID || centre_mode == PNPP_SCAN_BOX, PNPP_ERR_ARG,
                 "normalize_clouds: centre mode %d is none of PNPP_SCAN_NONE, _CENTROID, _BOX", centre_mode);
    PNPP_REQUIRE(scale_mode == PNPP_SCAN_NONE || scale_mode == PNPP_SCAN_SPHERE || scale_mode == PNPP_SCAN_BOX, PNPP_ERR_ARG,
                 "normalize_clouds: scale mode %d is none of PNPP_SCAN_NONE, _SPHERE, _BOX", scale_mode);
    ProfScope ps(as_stream(stream), "normalize_clouds_kernel B=%d N=%lld C=%d centre=%d scale=%d", B, (long long)N, C, centre_mode, scale_mode);
    hipLaunchKernelGGL(normalize_clouds_kernel, dim3((unsigned)B), dim3(kScanTile), 0, as_stream(stream), xyz_in, xyz_out, lengths, (int)N, C,
                       centre_mode, scale_mode, centre_out, scale_out);
    PNPP_CHECK_LAUNCH("normalize_clouds");
    return PNPP_OK;
}
