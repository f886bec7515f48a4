// knn_search.h -- the kNN search of knn_kernels.hip: one wavefront per query centre, knn_body over named steps.
//
// kNN grouping (models/base.py:29-35):
//   * the cloud is staged tile by tile (TILE points) into LDS as x[],y[],z[],|p|^2[] (SoA);
//   * every lane forms 64-bit keys (sortable(d) << 32 | n) for TILE/64 candidates in registers;
//   * prune: the k-th smallest of the 64 lane minima bounds the k-th smallest key of the tile from
//     above (k <= 64), and so does the previous best list's last entry; only keys <= that bound are
//     compacted (ballot + prefix popcount) into a small LDS pool -- typically 40-70 of 1024;
//   * select: every pooled key counts the pooled keys below it (broadcast LDS reads); rank < k
//     writes straight to its sorted slot.  Keys are unique (index in the low word), so ranks are too.
//   * pathological inputs (pool overflow: massive ties, or k > 64) fall back to k rounds of
//     "wave-min, owner retires its key".
// Output: neighbours in ascending (distance, index).
//
// The steps below are the body's vocabulary: load_query, form_keys, prune_bound, compact_pool, select_ranks, write_list, list_point and
// moments_epilogue (tile staging and the fallback are sections of knn_body itself).  Each is inlined into it; a step's contract names
// what it reads, what it writes in KnnLds and which of its values are the same in every lane of the wave (wave-uniform).  A step that
// touches the lists or the pool takes (L, wave, cur) and indexes the arrays itself -- handed a pointer into them instead, the compiler
// forms other addresses and the kernels' register counts move.  The lists live in best[wave][2][]: the tile loop reads
// half `cur` and writes half `cur ^ 1`, `cur` flips once per tile walked, and pass p starts on half p & 1 -- so after its tiles a pass
// leaves the previous pass's list alone, and the epilogues find pass p's list on half (p ^ tiles walked) & 1.
// Included after exact_dist.h's conditions are met: -ffp-contract=off and `#pragma clang fp contract(off)` in the including file.
#pragma once
#include "common.h"
#include "exact_dist.h"
#include "split_prims.h"

namespace pnpp {

constexpr int KNN_TILE = 1024;
constexpr int KNN_TILE_SMALL = 128;   // a cloud of at most this many candidates (a stacked level's centres): two keys per lane, not sixteen
constexpr int KNN_KMAX = 128;
constexpr int KNN_POOL = 256;
constexpr int KNN_PAIR_QPW = 2;
constexpr int KNN_MOM_PITCH = 16;     // == kMomPitch (wsf0_args.h): one moment partial per workgroup
constexpr unsigned long long KEY_MAX = ~0ull;

// centre != nullptr: the query of (b, q) is xyz[b, centre[b, q]] and the kernel also writes it to out_a / out_b (the
// caller's new_xyz and the copy kept for backward) -- the set-abstraction forward then needs no separate gather launch.
// gather != nullptr: the "cloud" of (b) is itself a gathered subset of xyz -- candidate p is xyz[b, gather[b, p]] (the centres
// of the level below, xyz holding Nsrc points per cloud): the neighbour search of a stacked level then needs neither the level
// below's output nor a launch of its own (knn_pair_kernel).
// mom != nullptr: the workgroup also sums the nine moments of rel = neighbour - centre over its queries' neighbourhoods (what
// rel_moments_kernel computes from idx in a launch of its own) and writes them as partial [b * gridDim-of-the-level + bx].
struct KnnJob {
    const float *new_xyz;      // explicit queries, or nullptr with `centre`
    const float *xyz;
    const int32_t *gather;     // (B, N) rows of xyz that form the candidate cloud, or nullptr (the cloud is xyz itself)
    int Nsrc;                  // points per cloud in xyz (== N without gather)
    int S, N, k;
    int32_t *idx;
    const int32_t *centre;
    float *out_a, *out_b;
    double *mom;               // [B * nblocks][KNN_MOM_PITCH] or nullptr
    int qpw;                   // queries per wave: 1, or 2 on a cloud of one tile (the tile is then staged once for eight queries)
    int nblocks;               // workgroups per cloud of this job
    const int32_t *lengths;    // ragged batch (RAGGED bodies only): cloud b's candidates are its first min(max(lengths[b], 1), N) rows
    int store_policy;          // StorePolicy bits (common.h): the moment partials are a statistics slab
};

struct alignas(16) KnnLds {   // one copy per workgroup, shared by the two instantiations of the body a pair kernel contains
    float sx[KNN_TILE], sy[KNN_TILE], sz[KNN_TILE], sn[KNN_TILE];
    unsigned long long best[4][2][KNN_KMAX];
    unsigned long long pool[4][KNN_POOL];
};

// k-th smallest (1-based, with multiplicity) of the 64 lanes' values, wave-uniform: built bit by bit from the top -- a bit is set when
// fewer than k lanes lie at or below the candidate with that bit clear and every lower bit set.  32 compare + ballot + popcount steps
// on the scalar unit instead of a 64-step readlane / compare / add chain on the vector unit.
__device__ __forceinline__ unsigned wave_kth_smallest_u32(unsigned v, int k) {
    unsigned t = 0u;
#pragma unroll
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = t | ((1u << bit) - 1u);
        if (__popcll(__ballot(v <= cand)) < k) t |= 1u << bit;
    }
    return t;
}

struct KnnQuery {
    float x, y, z, sq;   // the query point and |a|^2
};

// Query load: reads row q of cloud b's queries -- new_xyz, or xyz through centre (and, GATHER, through gather) -- and with a centre
// writes it to out_a / out_b from lanes 0-2.  Touches nothing in KnnLds; the result is wave-uniform.
template <bool GATHER>
__device__ __forceinline__ KnnQuery load_query(const float *__restrict__ new_xyz, const float *__restrict__ xyz, const int32_t *__restrict__ centre,
                                               const int32_t *__restrict__ gather, float *__restrict__ out_a, float *__restrict__ out_b,
                                               int Nsrc, int S, int b, int q, int lane) {
    const float *a = new_xyz + ((size_t)b * S + q) * 3;
    if (centre) {
        const int c = centre[(size_t)b * S + q];
        a = xyz + ((size_t)b * Nsrc + (GATHER ? gather[c] : c)) * 3;
    }
    const float ax = a[0], ay = a[1], az = a[2];
    const float sa = sq3_exact(ax, ay, az);
    if (centre && lane < 3) {
        const float v = lane == 0 ? ax : (lane == 1 ? ay : az);
        out_a[((size_t)b * S + q) * 3 + lane] = v;
        if (out_b) out_b[((size_t)b * S + q) * 3 + lane] = v;
    }
    return {ax, ay, az, sa};
}

// Key formation: reads the staged tile and, with `have`, the current list best[wave][cur] (the previous best rides along as up to two
// more candidates per lane); writes nothing in KnnLds.  key[] and the returned minimum of the lane's tile keys are per lane; Q, have, k
// and cur are wave-uniform.
template <int TILE>
__device__ __forceinline__ unsigned long long form_keys(const KnnLds &L, int wave, int cur, const KnnQuery Q, int t0, int cnt, int lane,
                                                        bool have, int k, unsigned long long (&key)[TILE / 64 + 2]) {
    constexpr int CPL = TILE / 64;              // candidates per lane per tile
    unsigned long long lmin = KEY_MAX;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int p = j * 64 + lane;
        key[j] = KEY_MAX;
        if (p < cnt) {
            float d = pair_dist_exact(Q.x, Q.y, Q.z, L.sx[p], L.sy[p], L.sz[p], Q.sq, L.sn[p]);
            key[j] = ((unsigned long long)f32_sortable(d) << 32) | (unsigned)(t0 + p);
        }
        lmin = key[j] < lmin ? key[j] : lmin;
    }
    key[CPL] = (have && lane < k) ? L.best[wave][cur][lane] : KEY_MAX;
    key[CPL + 1] = (have && lane + 64 < k) ? L.best[wave][cur][lane + 64] : KEY_MAX;
    return lmin;
}

// Pruning bound on the distance word: reads the lane minima and, with `have`, the last entry of best[wave][cur]; writes nothing.  The
// result is wave-uniform: no key above it can be among the k smallest.
__device__ __forceinline__ unsigned long long prune_bound(const KnnLds &L, int wave, int cur, unsigned long long lmin, int k, bool have) {
    unsigned long long T = KEY_MAX;
    if (k <= 64) T = ((unsigned long long)wave_kth_smallest_u32((unsigned)(lmin >> 32), k) << 32) | 0xffffffffull;
    if (have) {
        const unsigned long long last = L.best[wave][cur][k - 1];
        T = last < T ? last : T;
    }
    return T;
}

// Compaction of the survivors (key <= T) into pool[wave]: writes its first min(P, KNN_POOL) entries and returns P, the number of
// survivors (wave-uniform; P > KNN_POOL: the pool overflowed and holds only the first KNN_POOL).  lt_mask: the lanes below this one.
template <int NK>
__device__ __forceinline__ int compact_pool(KnnLds &L, int wave, const unsigned long long (&key)[NK], unsigned long long T,
                                            unsigned long long lt_mask) {
    int P = 0;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const bool in = key[j] <= T && key[j] != KEY_MAX;
        const unsigned long long mb = __ballot(in);
        const int pos = P + __popcll(mb & lt_mask);
        if (in && pos < KNN_POOL) L.pool[wave][pos] = key[j];
        P += __popcll(mb);
    }
    return P;
}

// Rank selection inside the pool (P <= KNN_POOL, wave-uniform): reads pool[wave][0, P), pads it with KEY_MAX (never below a pooled key)
// to a multiple of four entries, and writes the k smallest, sorted, to best[wave][cur ^ 1][0, k).  A step reads four entries with two
// 16-byte broadcasts that are in flight together.
__device__ __forceinline__ void select_ranks(KnnLds &L, int wave, int cur, int P, int k, int lane) {
    if (lane < 3 && P + lane < ((P + 3) & ~3)) L.pool[wave][P + lane] = KEY_MAX;
    const ulonglong2 *pool2 = reinterpret_cast<const ulonglong2 *>(L.pool[wave]);
    const int P2 = (P + 3) >> 2 << 1;
    for (int e0 = 0; e0 < P; e0 += 64) {
        const int e = e0 + lane;
        const unsigned long long mine = e < P ? L.pool[wave][e] : KEY_MAX;
        int r = 0;
#pragma unroll 2
        for (int j = 0; j < P2; j += 2) {
            const ulonglong2 u = pool2[j], v = pool2[j + 1];
            r += (u.x < mine ? 1 : 0) + (u.y < mine ? 1 : 0) + (v.x < mine ? 1 : 0) + (v.y < mine ? 1 : 0);
        }
        if (e < P && r < k) L.best[wave][cur ^ 1][r] = mine;
    }
}

// List write-out: reads list[0, k), writes the index words to the query's row o[0, k).  RAGGED: slots at or beyond the cloud's extent
// N repeat slot 0.
template <bool RAGGED>
__device__ __forceinline__ void write_list(const unsigned long long *list, int32_t *o, int k, int N, int lane) {
    for (int j = lane; j < k; j += 64) o[j] = (int32_t)(unsigned)(list[RAGGED && j >= N ? 0 : j] & 0xffffffffu);
}

// Coordinates of row n of the cloud, n taken from a selected list: from the staged tile when the cloud is one tile (it is then still
// in sx, sy, sz after the last pass), else from global memory.  Reads only; `staged` is wave-uniform.
__device__ __forceinline__ void list_point(bool staged, const float *sx, const float *sy, const float *sz, const float *cloud, unsigned n,
                                           float &nx, float &ny, float &nz) {
    if (staged) nx = sx[n], ny = sy[n], nz = sz[n];
    else nx = cloud[(size_t)n * 3], ny = cloud[(size_t)n * 3 + 1], nz = cloud[(size_t)n * 3 + 2];
}

}  // namespace pnpp

#include "knn_normals.h"   // the NRM hook of knn_body; its covariance uses list_point

namespace pnpp {

// Moments epilogue, the whole workgroup after its last pass (J.mom != nullptr): rel = neighbour - centre over the wave's neighbourhoods,
// the same float32 terms rel_moments_kernel forms from idx, summed in float64.  Reads every pass's list -- pass p began on half p & 1 of
// best[] and flipped once per tile, so it is on half (p ^ ntiles) & 1 -- and the staged tile or the cloud; reuses pool[wave] (free by
// now) for the wave's nine sums, one barrier, and threads 0-8 write the workgroup's partial.  Fixed order: lanes (butterfly), then the
// four waves in wave order.
template <int TILE, bool RAGGED>
__device__ __forceinline__ void moments_epilogue(const KnnJob &J, int bx, int b, int N, const float *cloud, KnnLds &L, int wave, int lane) {
    double m[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int ntiles = (N + TILE - 1) / TILE;
    for (int pass = 0; pass < J.qpw; ++pass) {
        const int q = (bx * J.qpw + pass) * 4 + wave;
        if (q >= J.S) continue;
        const float *a = J.centre ? J.xyz + ((size_t)b * J.Nsrc + J.centre[(size_t)b * J.S + q]) * 3 : J.new_xyz + ((size_t)b * J.S + q) * 3;
        const float ax = a[0], ay = a[1], az = a[2];
        const unsigned long long *list = L.best[wave][(pass ^ ntiles) & 1];
        for (int j = lane; j < J.k; j += 64) {
            const unsigned n = (unsigned)(list[RAGGED && j >= N ? 0 : j] & 0xffffffffu);
            float nx, ny, nz;
            list_point(N <= TILE, L.sx, L.sy, L.sz, cloud, n, nx, ny, nz);
            const float x = __fsub_rn(nx, ax), y = __fsub_rn(ny, ay), z = __fsub_rn(nz, az);
            m[0] += (double)x, m[1] += (double)y, m[2] += (double)z;
            m[3] += (double)__fmul_rn(x, x), m[4] += (double)__fmul_rn(x, y), m[5] += (double)__fmul_rn(x, z);
            m[6] += (double)__fmul_rn(y, y), m[7] += (double)__fmul_rn(y, z), m[8] += (double)__fmul_rn(z, z);
        }
    }
    double *red = reinterpret_cast<double *>(L.pool[wave]);
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        double v = m[c];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += shfl_xor_f64(v, o);
        if (lane == 0) red[c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const double *r0 = reinterpret_cast<const double *>(L.pool[0]), *r1 = reinterpret_cast<const double *>(L.pool[1]);
        const double *r2 = reinterpret_cast<const double *>(L.pool[2]), *r3 = reinterpret_cast<const double *>(L.pool[3]);
        sp_store(J.mom + ((size_t)b * J.nblocks + bx) * KNN_MOM_PITCH + threadIdx.x,
                 (r0[threadIdx.x] + r1[threadIdx.x]) + (r2[threadIdx.x] + r3[threadIdx.x]), (J.store_policy & ST_STAT_SLABS) != 0);
    }
}

// The body of every kNN kernel.  For each pass (query of the wave): load the query; for each tile: stage it (pass 0), form keys, bound,
// compact, then select or fall back; write the list, then the normals hook.  Then the epilogues.
// RAGGED: N below is the cloud's own extent Nv (one scalar load per workgroup); the host still sized TILE, qpw and the grid from the
// padded J.N, so Nv <= J.N tiles are walked, `cur` flips once per tile actually walked, and a list asked for more neighbours than
// the cloud has points (k > Nv, which the host refuses where it sees the lengths) repeats slot 0 in the slots >= Nv.
// NRM (with W): every point of the cloud is a query (new_xyz == xyz, S == J.N) and each pass ends with the covariance of the list it
// has just selected -- at the end of the pass, not after all of them, because best[][2][] keeps two passes' lists, so qpw is free on
// a cloud of one tile (qpw <= 64: pass p's covariance waits in lane p for the solve after the last pass).  idx is then optional.
// RAGGED: a query at or beyond Nv skips the search and writes zeros.
template <bool GATHER, int TILE, bool MOM, bool RAGGED = false, bool NRM = false>
__device__ __forceinline__ void knn_body(const KnnJob &J, const int bx, const int b, KnnLds &L, const KnnNormals *W = nullptr) {
    constexpr int NK = TILE / 64 + 2;           // keys a lane holds per tile: its candidates and two slots of the previous list
    const float *__restrict__ new_xyz = J.new_xyz;
    const float *__restrict__ xyz = J.xyz;
    const int32_t *__restrict__ centre = J.centre;
    const int32_t *__restrict__ gather = GATHER ? J.gather + (size_t)b * J.N : nullptr;
    int32_t *__restrict__ idx = J.idx;
    float *__restrict__ out_a = J.out_a, *__restrict__ out_b = J.out_b;
    const int S = J.S, k = J.k;
    int N = J.N;
    if constexpr (RAGGED) N = min(max(J.lengths[b], 1), N);   // wave-uniform: b is the workgroup's cloud
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const float *cloud = xyz + (size_t)b * J.Nsrc * 3;
    const int qpw = J.qpw;   // > 1 only with N <= TILE: the one tile staged in the first pass serves every pass

    if constexpr (NRM && RAGGED) {
        if (bx * qpw * 4 >= N) {   // the workgroup lies wholly beyond its cloud: its zeros, and no tile is staged
            for (int pass = 0; pass < qpw; ++pass) {
                const int q = (bx * qpw + pass) * 4 + wave;
                if (q < S) normals_zero_row(*W, idx, (size_t)b * S + q, k, lane);
            }
            return;
        }
    }

    [[maybe_unused]] double cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // NRM: lane p holds pass p's covariance
    for (int pass = 0; pass < qpw; ++pass) {
        const int q = (bx * qpw + pass) * 4 + wave;
        const bool active = q < S && (!NRM || q < N);  // wave-uniform
        KnnQuery Q{0.f, 0.f, 0.f, 0.f};
        if (active) Q = load_query<GATHER>(new_xyz, xyz, centre, gather, out_a, out_b, J.Nsrc, S, b, q, lane);
        int cur = pass & 1;  // which half of best[] holds the current list (alternating, so a pass leaves the previous pass's result alone)
        bool have = false;   // best[cur][0..k) is valid (wave-uniform)

        for (int t0 = 0; t0 < N; t0 += TILE) {
            const int cnt = min(TILE, N - t0);
            if (pass == 0) {
                if (t0 > 0) __syncthreads();  // previous tile fully consumed
                // ---- stage the tile, all 256 threads: one point per thread and step (three floats of a row; gathered clouds: of the
                // listed row), every load of the thread requested before the first is used; |p|^2 comes from the registers, so the
                // tile needs one barrier.  (In the body, not a step: as a function it costs knn_pair_kernel two registers.) ----
                constexpr int SPT = (TILE + 255) / 256;     // staged points per thread per tile
                float px[SPT], py[SPT], pz[SPT];
#pragma unroll
                for (int i = 0; i < SPT; ++i) {
                    const int p = min((int)threadIdx.x + 256 * i, cnt - 1);
                    const float *s = cloud + (size_t)(GATHER ? gather[t0 + p] : t0 + p) * 3;
                    px[i] = s[0], py[i] = s[1], pz[i] = s[2];
                }
#pragma unroll
                for (int i = 0; i < SPT; ++i) {
                    const int p = threadIdx.x + 256 * i;
                    if (p < cnt) L.sx[p] = px[i], L.sy[p] = py[i], L.sz[p] = pz[i], L.sn[p] = sq3_exact(px[i], py[i], pz[i]);
                }
                __syncthreads();
            }
            if (!active) continue;

            unsigned long long key[NK];
            const unsigned long long lmin = form_keys<TILE>(L, wave, cur, Q, t0, cnt, lane, have, k, key);
            const unsigned long long T = prune_bound(L, wave, cur, lmin, k, have);
            const int P = compact_pool<NK>(L, wave, key, T, lt_mask);
            if (P <= KNN_POOL) {
                select_ranks(L, wave, cur, P, k, lane);
            } else {
                // ---- fallback (pool overflow): k rounds of wave-min extraction over everything this lane holds; each round's minimum
                // is wave-uniform and lane 0 writes it to best[wave][cur ^ 1].  (In the body, not a step: as a function over key[] it
                // changes knn_normals_kernel's register count.) ----
                unsigned long long fmin = lmin;   // the minimum of the lane's tile keys, then of its two list slots
#pragma unroll
                for (int j = NK - 2; j < NK; ++j) fmin = key[j] < fmin ? key[j] : fmin;
                for (int it = 0; it < k; ++it) {
                    const unsigned long long w = wave_min_u64(fmin);
                    if (lane == 0) L.best[wave][cur ^ 1][it] = w;
                    if (fmin == w && w != KEY_MAX) {  // keys are unique: exactly one owner
                        unsigned long long m2 = KEY_MAX;
#pragma unroll
                        for (int j = 0; j < NK; ++j) {
                            if (key[j] == w) key[j] = KEY_MAX;
                            m2 = key[j] < m2 ? key[j] : m2;
                        }
                        fmin = m2;
                    }
                }
            }
            cur ^= 1;
            have = true;
        }
        if (active && (!NRM || idx)) write_list<RAGGED>(L.best[wave][cur], idx + ((size_t)b * S + q) * k, k, N, lane);
        if constexpr (NRM) {
            if (active) {
                double c[6];
                normals_covariance<RAGGED>(L.best[wave][cur], k, N, N <= TILE, L.sx, L.sy, L.sz, cloud, Q.x, Q.y, Q.z, lane, c);
#pragma unroll
                for (int i = 0; i < 6; ++i) cov[i] = lane == pass ? c[i] : cov[i];
            } else if (RAGGED && q < S) normals_zero_row(*W, idx, (size_t)b * S + q, k, lane);
        }
    }
    if constexpr (NRM) {
        const int q = (bx * qpw + lane) * 4 + wave;   // lane p: the wave's query of pass p
        if (lane < qpw && q < S && q < N) {
            const float *a = xyz + ((size_t)b * S + q) * 3;
            normals_solve_store(*W, cov, W->ref ? W->ref + (size_t)b * 3 : nullptr, (size_t)b * S + q, a[0], a[1], a[2]);
        }
    }
    if constexpr (MOM) {
        if (J.mom) moments_epilogue<TILE, RAGGED>(J, bx, b, N, cloud, L, wave, lane);
    }
}

}  // namespace pnpp
