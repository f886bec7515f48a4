// sampling_kernels.hip -- centre sampling for gfx950 (MI355X): farthest-point sampling, the Philox centre draws and the bank
// subsampler; their launchers and C entries.  The Philox rounds and the draw's body are sampler_device.h (the step tails share them).
// Compiled with -ffp-contract=off (exact_dist.h): the farthest-point distances are the reference's exact float32 sequence.
#include "common.h"
#include "sampler_device.h"

#pragma clang fp contract(off)

#include "exact_dist.h"

namespace pnpp {

// Wave-wide maximum of a 64-bit key, result in every lane.  Six dependent ds_bpermute round trips (what __shfl_xor compiles
// to) are most of a farthest-point round; this is the DPP form: an inclusive row scan (row_shr 1, 2, 4, 8 inside the rows of
// 16 lanes, shifted-in lanes keep their own value), row_bcast15 / row_bcast31 to fold the four rows, lane 63 read back
// through the scalar unit -- VALU latency only.
__device__ __forceinline__ unsigned long long wave_max_u64_dpp(unsigned long long v) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#define PNPP_DPP_MAX_STEP(CTRL, ROWMASK)                                                                              \
    {                                                                                                                 \
        const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp((int)lo, (int)lo, CTRL, ROWMASK, 0xf, false);      \
        const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp((int)hi, (int)hi, CTRL, ROWMASK, 0xf, false);      \
        const bool take = ohi > hi || (ohi == hi && olo > lo);                                                        \
        lo = take ? olo : lo, hi = take ? ohi : hi;                                                                   \
    }
    PNPP_DPP_MAX_STEP(0x111, 0xf)  // row_shr:1
    PNPP_DPP_MAX_STEP(0x112, 0xf)  // row_shr:2
    PNPP_DPP_MAX_STEP(0x114, 0xf)  // row_shr:4
    PNPP_DPP_MAX_STEP(0x118, 0xf)  // row_shr:8   -> lane 15 of every row holds its row's maximum
    PNPP_DPP_MAX_STEP(0x142, 0xa)  // row_bcast15 -> rows 1 and 3 fold in the row below
    PNPP_DPP_MAX_STEP(0x143, 0xc)  // row_bcast31 -> rows 2 and 3 fold in lane 31: lane 63 holds the wave's maximum
#undef PNPP_DPP_MAX_STEP
    const unsigned rlo = (unsigned)__builtin_amdgcn_readlane((int)lo, 63), rhi = (unsigned)__builtin_amdgcn_readlane((int)hi, 63);
    return ((unsigned long long)rhi << 32) | rlo;
}

// ---------------------------------------------------------------------------------------------
// farthest point sampling (PointNet++Demo.py:8-29): one workgroup per cloud.
//
// The algorithm is a chain of npoint dependent rounds (distance update over all N points, arg-max, next centre), so its
// time is npoint x (latency of one round); a round is short enough (< 1 us up to N ~ 16k) that handing the arg-max
// between workgroups through memory (>= 1 us per hop) would lengthen it -- a cloud therefore stays on ONE CU and the
// round is made short instead:
//   * every thread keeps its PPT points (x, y, z, running minimum) in REGISTERS for the whole kernel: a round touches
//     the LDS only for the T/64 per-wave winners, and N is bounded by the register file (T x PPT points), not by 16 bytes
//     of LDS per point; points beyond T x PPT (N > 16384) live in the LDS as before (the "tail", up to 160 KiB / 16 B more);
//   * the winner's coordinates travel with its key: the lane that owns a wave's maximum writes (key, x, y, z) to its
//     wave's slot, so the next centre needs no lookup by index (one barrier per round, slots double-buffered);
//   * ties: key = (distance bits << 32) | ~index, i.e. the FIRST maximum, as torch.max(distance, -1)[1] (line 28).
// Distances are the reference's exact float32 sequence ((dx^2 + dy^2) + dz^2, no FMA) -> indices are bit-exact.
// ---------------------------------------------------------------------------------------------
// RAGGED: register and tail slots at or beyond the cloud's own extent Nv = min(max(lengths[b], 1), N) are slots past the cloud
// (distance -1, coordinates of row Nv - 1); start[b] < Nv is the caller's to keep.  T / PPT / ntail come from the padded N.
template <int T, int PPT, bool RAGGED>
__global__ void __launch_bounds__(T) fps_kernel(const float *__restrict__ xyz, const int Npad, int npoint,
                                                const int32_t *__restrict__ start, int32_t *__restrict__ out, int ntail,
                                                const int32_t *__restrict__ lengths) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NW = T / 64;
    // one LDS object (a second __shared__ array beside a dynamic one can cost a vmcnt(0) per read, guide 5.4 item 4a):
    // [2][NW] keys (u64) | [2][NW][4] winner coordinates | tail: x[ntail] y[ntail] z[ntail] d[ntail]
    unsigned long long *wkey = reinterpret_cast<unsigned long long *>(lds);
    float *wxyz = lds + 2 * 2 * NW;
    float *sx = wxyz + 2 * NW * 4, *sy = sx + ntail, *sz = sy + ntail, *sd = sz + ntail;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *cloud = xyz + (size_t)b * Npad * 3;
    int N = Npad;
    if constexpr (RAGGED) N = min(max(lengths[b], 1), Npad);
    float px[PPT], py[PPT], pz[PPT], pd[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int p = tid + j * T, pc = p < N ? p : N - 1;
        px[j] = cloud[pc * 3 + 0], py[j] = cloud[pc * 3 + 1], pz[j] = cloud[pc * 3 + 2];
        pd[j] = p < N ? 1e10f : -1.f;   // a slot past the cloud: min(d, -1) = -1 never beats a real (non-negative) distance
    }
    for (int q = tid; q < ntail; q += T) {
        const int p = T * PPT + q, pc = RAGGED && p >= N ? N - 1 : p;
        sx[q] = cloud[pc * 3 + 0], sy[q] = cloud[pc * 3 + 1], sz[q] = cloud[pc * 3 + 2], sd[q] = RAGGED && p >= N ? -1.f : 1e10f;
    }
    int far = start[b];
    float cx = cloud[far * 3 + 0], cy = cloud[far * 3 + 1], cz = cloud[far * 3 + 2];
    if (ntail) __syncthreads();

    for (int it = 0; it < npoint; ++it) {
        if (tid == 0) out[(size_t)b * npoint + it] = far;
        // inside a thread the points are visited in ascending index, so a strict float compare keeps the FIRST maximum;
        // distances are non-negative, so their bit patterns order like unsigned integers -- the 64-bit key
        // (distance bits << 32) | ~index is only built once per thread, for the cross-lane reduction
        float bv = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bp = 0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const float cur = fminf(direct_dist_exact(px[j], py[j], pz[j], cx, cy, cz), pd[j]);   // NaN distance: keeps pd, like dist < distance
            pd[j] = cur;
            const bool w = cur > bv;
            bv = w ? cur : bv, bp = w ? tid + j * T : bp, bx = w ? px[j] : bx, by = w ? py[j] : by, bz = w ? pz[j] : bz;
        }
        for (int q = tid; q < ntail; q += T) {
            const float x = sx[q], y = sy[q], z = sz[q];
            const float cur = fminf(direct_dist_exact(x, y, z, cx, cy, cz), sd[q]);
            sd[q] = cur;
            const bool w = cur > bv;
            bv = w ? cur : bv, bp = w ? T * PPT + q : bp, bx = w ? x : bx, by = w ? y : by, bz = w ? z : bz;
        }
        // a thread without a valid point (bv < 0) contributes key 0, below every real key (~index is never 0)
        const unsigned long long bestk =
            bv < 0.f ? 0ull : ((unsigned long long)__float_as_uint(bv) << 32) | (unsigned)(0xffffffffu - (unsigned)bp);
        const unsigned long long wk = wave_max_u64_dpp(bestk);
        if (bestk == wk && (wk != 0ull || lane == 0)) {   // keys carry the point index: exactly one lane of the wave holds the maximum
            wkey[(it & 1) * NW + wave] = wk;
            float *w4 = wxyz + ((it & 1) * NW + wave) * 4;
            w4[0] = bx, w4[1] = by, w4[2] = bz;
        }
        __syncthreads();
        // (folding the NW slots with a second DPP maximum + readlane instead of reading them all was measured slower:
        // 98.6 vs 80.3 us at N = 1024 -- the scalar round trip is longer than two LDS round trips)
        unsigned long long g = 0;
        int gw = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const unsigned long long o = wkey[(it & 1) * NW + w];
            const bool win = o > g;
            g = win ? o : g, gw = win ? w : gw;
        }
        far = (int)(0xffffffffu - (unsigned)(g & 0xffffffffu));
        const float *w4 = wxyz + ((it & 1) * NW + gw) * 4;
        cx = w4[0], cy = w4[1], cz = w4[2];
    }
}

// ---------------------------------------------------------------------------------------------
// device-side centre sampling: uniform random ordered subset (replaces B host randperm calls).
// key(n) = Philox4x32-10(counter = (n, b, stream_lo, stream_hi), key = seed); rank by (key, n);
// out[rank] = n for rank < npoint.  Fully deterministic (a pure function of seed, stream id and cloud).
// ---------------------------------------------------------------------------------------------
// (philox_key and the sampling body: sampler_device.h)
template <bool RAGGED>
__global__ void __launch_bounds__(256) sample_random_kernel(unsigned seed_lo, unsigned seed_hi, unsigned str_lo,
                                                            unsigned str_hi, unsigned long long *__restrict__ str_dev,
                                                            int N, int npoint, int32_t *__restrict__ out, int B1, int N2,
                                                            int npoint2, int32_t *__restrict__ out2, const int32_t *__restrict__ lengths) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long cand[];
    __shared__ int nc_s;
    sample_random_body<RAGGED>(seed_lo, seed_hi, str_lo, str_hi, str_dev, N, npoint, out, B1, N2, npoint2, out2, blockIdx.x, gridDim.x, cand,
                               nc_s, lengths);
}

// ---------------------------------------------------------------------------------------------
// on-device point subsampling for the data path (dataloader_*: sample_pts / np.random.choice(len, num, replace=len<num)):
// a bank of full clouds stays resident in HBM as (n_clouds, Lmax, 3) + lengths; one workgroup per batch slot draws
// `num` rows of its cloud -- an ordered uniform subset without replacement when the cloud has at least `num` points
// (same key + rank scheme as sample_random_kernel), uniform draws with replacement otherwise -- and writes the
// coordinates straight into the batch tensor.  Pure function of (seed, stream id, slot); empty clouds give zeros.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
subsample_points_kernel(unsigned seed_lo, unsigned seed_hi, unsigned str_lo, unsigned str_hi,
                        const float *__restrict__ bank, const int32_t *__restrict__ lengths,
                        const int32_t *__restrict__ cloud_ids, int Lmax, int num, float *__restrict__ out, int cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long cand[];
    // gridDim.y workgroups share one batch slot: each builds the slot's whole candidate list (cheap: one Philox call per
    // point) and ranks / gathers every gridDim.y-th candidate -- ranks do not depend on the order candidates were compacted in
    const int b = blockIdx.x, part = blockIdx.y, nparts = gridDim.y;
    const int cloud = cloud_ids ? cloud_ids[b] : b;
    const int L = min(lengths[cloud], Lmax);
    const float *src = bank + (size_t)cloud * Lmax * 3;
    float *dst = out + (size_t)b * num * 3;
    if (L <= 0) {
        for (int j = part * 256 + threadIdx.x; j < 3 * num; j += 256 * nparts) dst[j] = 0.f;
        return;
    }
    if (L < num) {  // with replacement: index = floor(u * L), u from the 32-bit Philox word
        for (int j = part * 256 + threadIdx.x; j < num; j += 256 * nparts) {
            const unsigned u = philox_key((unsigned)j, (unsigned)b, str_lo, str_hi, seed_lo, seed_hi);
            const int n = (int)(((unsigned long long)u * (unsigned long long)L) >> 32);
            dst[3 * j] = src[3 * n], dst[3 * j + 1] = src[3 * n + 1], dst[3 * j + 2] = src[3 * n + 2];
        }
        return;
    }
    const double keep = (num + 4.0 * sqrt((double)num) + 16.0) / (double)L;
    unsigned cut = keep >= 1.0 ? 0xffffffffu : (unsigned)(keep * 4294967296.0);
    // Compaction without atomics: wave w scans the points [w L/4, (w+1) L/4) and appends its survivors to its own segment
    // of the list, so the list -- positions included -- is the same in every workgroup of the slot: position p of the
    // concatenated segments belongs to part p / 256 % nparts.  Segments are padded to an even length with a word above every key.
    // The table holds `cap` words per segment whatever the cloud's length (clouds of millions of points draw through the same
    // few thousand words): a cut that leaves fewer than num keys, or more than a segment holds, is bisected -- the result (the
    // num smallest (key, index) words) never depends on where the cut ends up.
    __shared__ int cnt_s[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int seg = cap;                                    // capacity of one segment (even)
    const int lo = wave * ((L + 3) / 4), hi = min(L, lo + (L + 3) / 4);
    unsigned long long *mycand = cand + (size_t)wave * seg;
    unsigned cut_lo = 0u, cut_hi = 0xffffffffu;             // keys <= cut_lo are too few, keys <= cut_hi may not fit
    for (int round = 0;; ++round) {
        int cnt = 0;
        for (int n0 = lo; n0 < hi; n0 += 64) {
            const int n = n0 + lane;
            const unsigned k = n < hi ? philox_key((unsigned)n, (unsigned)b, str_lo, str_hi, seed_lo, seed_hi) : 0u;
            const bool keepit = n < hi && k <= cut;
            const unsigned long long vote = __ballot(keepit);
            const int pos = cnt + __popcll(vote & ((1ull << lane) - 1ull));
            if (keepit && pos < seg - 1) mycand[pos] = ((unsigned long long)k << 32) | (unsigned)n;
            cnt += __popcll(vote);
        }
        if (lane == 0) {
            if ((cnt & 1) && cnt < seg) mycand[cnt] = ~0ull;
            cnt_s[wave] = cnt;
        }
        __syncthreads();
        const int total = cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3];
        const bool fits = cnt_s[0] < seg && cnt_s[1] < seg && cnt_s[2] < seg && cnt_s[3] < seg;
        if ((total >= num && fits) || round >= 40) break;   // uniform (round bound: never reached, 32 bisections settle any cut)
        if (total < num) {                                  // too few keys under the cut (a > 5 sigma event): raise it
            cut_lo = cut;
            if (cut_hi != 0xffffffffu) cut = cut_lo + (cut_hi - cut_lo) / 2u;          // between a too-small and a too-large cut
            else if (4 * (seg - 2) >= L + 8) cut = 0xffffffffu;                        // the whole cloud fits the table: take it
            else cut = cut > 0x7fffffffu ? 0xffffffffu : 2u * cut + 1u;                // never overflowed yet: double
        } else {                                            // a segment overflowed: lower it
            cut_hi = cut;
            cut = cut_lo + (cut_hi - cut_lo) / 2u;
        }
        __syncthreads();
    }
    const int c0 = cnt_s[0], c1 = cnt_s[1], c2n = cnt_s[2], c3 = cnt_s[3], nc = c0 + c1 + c2n + c3;
    const ulonglong2 *pairs = reinterpret_cast<const ulonglong2 *>(cand);
    for (int p = part * 256 + threadIdx.x; p < nc; p += 256 * nparts) {
        int w = 0, q = p;                                  // position p -> (segment, index)
        if (q >= c0) { q -= c0, w = 1; if (q >= c1) { q -= c1, w = 2; if (q >= c2n) q -= c2n, w = 3; } }
        const unsigned long long mine = cand[(size_t)w * seg + q];
        int rank = 0;
#pragma unroll
        for (int sgm = 0; sgm < 4; ++sgm) {
            const int np = (cnt_s[sgm] + 1) >> 1;
            const ulonglong2 *c2 = pairs + (size_t)sgm * (seg >> 1);
#pragma unroll 4
            for (int jj = 0; jj < np; ++jj) {             // one 16-byte LDS broadcast per two candidates
                const ulonglong2 o = c2[jj];
                rank += (o.x < mine) + (o.y < mine);
            }
        }
        if (rank < num) {
            const int n = (int)(unsigned)mine;
            dst[3 * rank] = src[3 * n], dst[3 * rank + 1] = src[3 * n + 1], dst[3 * rank + 2] = src[3 * n + 2];
        }
    }
}

}  // namespace pnpp

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace pnpp;

template <bool RAGGED>
static int fps_impl(const float *xyz, int B, int N, const int32_t *lengths, int npoint, const int32_t *start, int32_t *out, void *stream) {
    PNPP_REQUIRE(xyz && start && out, PNPP_ERR_ARG, "fps: null pointer");
    PNPP_REQUIRE(B > 0 && N > 0 && npoint > 0, PNPP_ERR_ARG, "fps: non-positive size");
    // npoint > N is legal, as in the reference (PointNet++Demo.py:8-29): once every distance is 0 the first maximum is point 0
    hipStream_t st = as_stream(stream);
    // points per thread live in registers; clouds beyond 1024 x 16 points keep the rest in the LDS (16 bytes per point)
    constexpr int kRegPoints = 1024 * 16, kTailMax = (160 * 1024 - 2048) / 16;   // 1 KiB of winner slots at T = 1024
    PNPP_REQUIRE(N <= kRegPoints + kTailMax, PNPP_ERR_ARG, "fps: N=%d exceeds the %d points one CU can hold (registers + LDS)", N,
                 kRegPoints + kTailMax);
    const int ntail = N > kRegPoints ? N - kRegPoints : 0;
    auto go = [&](auto kfn, int T) {
        const size_t lds = ((size_t)2 * 2 * (T / 64) + (size_t)2 * (T / 64) * 4 + (size_t)4 * ntail) * sizeof(float);
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        ProfScope ps(st, "fps_kernel<%d> B=%d N=%d npoint=%d%s", T, B, N, npoint, RAGGED ? " ragged" : "");
        hipLaunchKernelGGL(kfn, dim3(B), dim3(T), lds, st, xyz, N, npoint, start, out, ntail, lengths);
    };
    if (N <= 1024) go(fps_kernel<256, 4, RAGGED>, 256);
    else if (N <= 2048) go(fps_kernel<256, 8, RAGGED>, 256);
    else if (N <= 4096) go(fps_kernel<512, 8, RAGGED>, 512);
    else if (N <= 8192) go(fps_kernel<1024, 8, RAGGED>, 1024);
    else go(fps_kernel<1024, 16, RAGGED>, 1024);
    PNPP_CHECK_LAUNCH("fps");
    return PNPP_OK;
}

extern "C" int pnpp_fps(const float *xyz, int B, int N, int npoint, const int32_t *start, int32_t *out, void *stream) {
    return fps_impl<false>(xyz, B, N, nullptr, npoint, start, out, stream);
}
extern "C" int pnpp_fps_ragged(const float *xyz, int B, int N, const int32_t *lengths, int npoint, const int32_t *start, int32_t *out,
                               void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "fps_ragged: null lengths");
    return fps_impl<true>(xyz, B, N, lengths, npoint, start, out, stream);
}

// one launch of sample_random_kernel, ragged (lengths != nullptr: of the first draw) or not
static void sample_random_launch(int grid, size_t lds, void *stream, uint64_t seed, uint64_t sid, uint64_t *stream_id_dev, int N1, int npoint1,
                                 int32_t *out1, int B1, int N2, int npoint2, int32_t *out2, const int32_t *lengths) {
    unsigned long long *dev = reinterpret_cast<unsigned long long *>(stream_id_dev);
    const unsigned s0 = (unsigned)seed, s1 = (unsigned)(seed >> 32), i0 = (unsigned)sid, i1 = (unsigned)(sid >> 32);
    const auto kfn = lengths ? sample_random_kernel<true> : sample_random_kernel<false>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, as_stream(stream), s0, s1, i0, i1, dev, N1, npoint1, out1, B1, N2, npoint2, out2, lengths);
}

static int sample_random_impl(uint64_t seed, uint64_t stream_id, uint64_t *stream_id_dev, int B, int N, int npoint,
                              int32_t *out, void *stream, const int32_t *lengths = nullptr) {
    PNPP_REQUIRE(out, PNPP_ERR_ARG, "sample_random: null pointer");
    PNPP_REQUIRE(B > 0 && N > 0 && npoint > 0, PNPP_ERR_ARG, "sample_random: non-positive size");
    PNPP_REQUIRE(npoint <= N, PNPP_ERR_RANGE, "sample_random: npoint=%d > N=%d", npoint, N);
    PNPP_REQUIRE((size_t)(N + 1) * 8 <= 128 * 1024, PNPP_ERR_ARG, "sample_random: N=%d too large", N);
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "sample_random: batch exceeds grid limit");
    const size_t lds = (size_t)(N + 1) * sizeof(unsigned long long);
    ProfScope ps(as_stream(stream), "sample_random_kernel B=%d N=%d npoint=%d%s", B, N, npoint, lengths ? " ragged" : "");
    sample_random_launch(B, lds, stream, seed, stream_id, stream_id_dev, N, npoint, out, 0, 0, 0, nullptr, lengths);
    PNPP_CHECK_LAUNCH("sample_random");
    return PNPP_OK;
}

extern "C" int pnpp_sample_random(uint64_t seed, uint64_t stream_id, int B, int N, int npoint, int32_t *out, void *stream) {
    return sample_random_impl(seed, stream_id, nullptr, B, N, npoint, out, stream);
}
extern "C" int pnpp_sample_random_ragged(uint64_t seed, uint64_t stream_id, int B, int N, const int32_t *lengths, int npoint, int32_t *out,
                                         void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "sample_random_ragged: null lengths");
    return sample_random_impl(seed, stream_id, nullptr, B, N, npoint, out, stream, lengths);
}

extern "C" int pnpp_sample_random_dev(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N, int npoint,
                                      int32_t *out, void *stream) {
    PNPP_REQUIRE(stream_id_dev, PNPP_ERR_ARG, "sample_random_dev: null counter pointer");
    return sample_random_impl(seed, offset, stream_id_dev, B, N, npoint, out, stream);
}
extern "C" int pnpp_sample_random_dev_ragged(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N, const int32_t *lengths,
                                             int npoint, int32_t *out, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "sample_random_dev_ragged: null lengths");
    PNPP_REQUIRE(stream_id_dev, PNPP_ERR_ARG, "sample_random_dev: null counter pointer");
    return sample_random_impl(seed, offset, stream_id_dev, B, N, npoint, out, stream, lengths);
}

static int sample_random_dev2_impl(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N1, const int32_t *lengths, int npoint1,
                                   int32_t *out1, int N2, int npoint2, int32_t *out2, void *stream) {
    PNPP_REQUIRE(stream_id_dev && out1 && out2, PNPP_ERR_ARG, "sample_random_dev2: null pointer");
    PNPP_REQUIRE(B > 0 && N1 > 0 && npoint1 > 0 && N2 > 0 && npoint2 > 0, PNPP_ERR_ARG, "sample_random_dev2: non-positive size");
    PNPP_REQUIRE(npoint1 <= N1 && npoint2 <= N2, PNPP_ERR_RANGE, "sample_random_dev2: npoint exceeds N");
    const int Nmax = N1 > N2 ? N1 : N2;
    PNPP_REQUIRE((size_t)(Nmax + 1) * 8 <= 128 * 1024, PNPP_ERR_ARG, "sample_random_dev2: N=%d too large", Nmax);
    PNPP_REQUIRE(2 * B <= 65535, PNPP_ERR_ARG, "sample_random_dev2: batch exceeds grid limit");
    const size_t lds = (size_t)(Nmax + 1) * sizeof(unsigned long long);
    ProfScope ps(as_stream(stream), "sample_random_kernel B=%d N=%d npoint=%d + N=%d npoint=%d%s", B, N1, npoint1, N2, npoint2,
                 lengths ? " ragged" : "");
    sample_random_launch(2 * B, lds, stream, seed, offset, stream_id_dev, N1, npoint1, out1, B, N2, npoint2, out2, lengths);
    PNPP_CHECK_LAUNCH("sample_random_dev2");
    return PNPP_OK;
}

extern "C" int pnpp_sample_random_dev2(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N1, int npoint1,
                                       int32_t *out1, int N2, int npoint2, int32_t *out2, void *stream) {
    return sample_random_dev2_impl(seed, stream_id_dev, offset, B, N1, nullptr, npoint1, out1, N2, npoint2, out2, stream);
}
extern "C" int pnpp_sample_random_dev2_ragged(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N1, const int32_t *lengths,
                                              int npoint1, int32_t *out1, int N2, int npoint2, int32_t *out2, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "sample_random_dev2_ragged: null lengths");
    return sample_random_dev2_impl(seed, stream_id_dev, offset, B, N1, lengths, npoint1, out1, N2, npoint2, out2, stream);
}

extern "C" int pnpp_subsample_points(uint64_t seed, uint64_t stream_id, const float *bank, const int32_t *lengths,
                                     const int32_t *cloud_ids, int B, int Lmax, int num, float *out, void *stream) {
    PNPP_REQUIRE(bank && lengths && out, PNPP_ERR_ARG, "subsample_points: null pointer");
    PNPP_REQUIRE(B > 0 && Lmax > 0 && num > 0, PNPP_ERR_ARG, "subsample_points: non-positive size");
    // four LDS segments of `cap` words: the whole cloud when it is short, else room for four times the keys the cut is expected
    // to keep (num + 4 sqrt(num) + 16, spread over the segments) -- independent of the cloud's length
    const long long want = 4ll * (long long)(num + 4.0 * sqrt((double)num) + 16.0) + 64;
    long long per_seg = ((long long)Lmax + 3) / 4 + 4;
    if (per_seg > want / 4 + 64) per_seg = want / 4 + 64;
    const int cap = (int)((per_seg + 1) & ~1ll);
    const size_t lds = (size_t)4 * cap * sizeof(unsigned long long);
    PNPP_REQUIRE(lds <= 128 * 1024, PNPP_ERR_ARG, "subsample_points: num=%d needs %zu bytes of LDS (<= 128 KB)", num, lds);
    static size_t granted = 0;
    if (lds > 48 * 1024 && lds > granted) {
        (void)hipFuncSetAttribute((const void *)subsample_points_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        granted = lds;
    }
    // the rank-by-counting pass is quadratic in the ~num survivors: spread a slot over several workgroups until the chip is full
    int nparts = 1;
    while (nparts < 8 && (long long)B * nparts * 2 <= 512 && num >= 128 * nparts * 2) nparts *= 2;
    ProfScope ps(as_stream(stream), "subsample_points_kernel B=%d Lmax=%d num=%d parts=%d", B, Lmax, num, nparts);
    hipLaunchKernelGGL(subsample_points_kernel, dim3(B, nparts), dim3(256), lds, as_stream(stream), (unsigned)seed,
                       (unsigned)(seed >> 32), (unsigned)stream_id, (unsigned)(stream_id >> 32), bank, lengths, cloud_ids, Lmax,
                       num, out, cap);
    PNPP_CHECK_LAUNCH("subsample_points");
    return PNPP_OK;
}
