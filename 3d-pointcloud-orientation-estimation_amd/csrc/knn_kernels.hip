// knn_kernels.hip -- the kNN kernels for gfx950 (MI355X): the plain search, the two stacked levels' searches in one launch, and the
// search with the normals epilogue; their launchers and C entries.  The search itself is knn_body (knn_search.h).
//
// Like every index kernel these are integer-, compare- or copy-bound (HBM/LDS bound, no MFMA): coalesced xyz reads, candidate tiles
// staged once per workgroup in LDS (SoA, conflict-free), one 64-lane wavefront per query, wave shuffles for the selection reductions.
// Compiled with -ffp-contract=off (exact_dist.h).
#include "common.h"
#include "wsf0_args.h"

#pragma clang fp contract(off)

#include "knn_search.h"

namespace pnpp {

template <bool RAGGED>
__global__ void __launch_bounds__(256) knn_kernel(const KnnJob J) {
    __shared__ KnnLds L;
    knn_body<false, KNN_TILE, false, RAGGED>(J, blockIdx.x, blockIdx.y, L);
}

// Normals of every point of the cloud: the search above with S == N queries and the normals epilogue per query (KnnNormals).
template <bool RAGGED>
__global__ void __launch_bounds__(256) knn_normals_kernel(const KnnJob J, const KnnNormals W) {
    __shared__ KnnLds L;
    knn_body<false, KNN_TILE, false, RAGGED, true>(J, blockIdx.x, blockIdx.y, L, &W);
}

// The neighbour searches of two stacked levels in ONE launch (they are independent once both levels' centre indices are drawn:
// level 2 searches among level 1's centres, which are rows of the same cloud).  blockIdx.x < nb2: level 2, else level 1.
// 5 workgroups per CU (<= 96 registers): 32 clouds x (32 + 8) workgroups = 1,280 are then all resident at once on 256 CUs -- at 4 per
// CU the last 256 start only when a slot frees up and the launch takes a round and a half (measured: 21.1 us against 12.6 + 7.0 for
// the two separate launches).  The short level-2 workgroups come first.  TILE2: level 2's tile (KNN_TILE_SMALL when its cloud fits).
// RAGGED: level 1 reads its cloud's length; level 2 searches level 1's centres, which are uniform.
template <int TILE2, bool RAGGED>
__global__ void __launch_bounds__(256, 5) knn_pair_kernel(const KnnJob J1, const KnnJob J2, int nb2) {
    __shared__ KnnLds L;
    if ((int)blockIdx.x < nb2) knn_body<true, TILE2, false>(J2, blockIdx.x, blockIdx.y, L);
    else knn_body<false, KNN_TILE, true, RAGGED>(J1, blockIdx.x - nb2, blockIdx.y, L);
}

// ---------------------------------------------------------------------------------------------
// host launchers (internal C++ API, used by the C ABI and by the set-abstraction orchestrator)
// ---------------------------------------------------------------------------------------------
// lengths != nullptr (here and in the launchers below): a ragged batch, cloud b's candidates are its first lengths[b] rows; the size
// checks stay those of the padded N (the device cannot refuse k > lengths[b]: see knn_body)

// One single-level search from a filled job: explicit queries (new_xyz) or gathered centres (centre, out_a).
static int launch_knn_job(const KnnJob &J, int B, hipStream_t st) {
    PNPP_REQUIRE(J.xyz && J.idx && (J.centre ? J.out_a != nullptr : J.new_xyz != nullptr), PNPP_ERR_ARG, "knn: null pointer");
    PNPP_REQUIRE(B > 0 && J.S > 0 && J.N > 0 && J.k > 0, PNPP_ERR_ARG, "knn: non-positive size (B=%d S=%d N=%d k=%d)", B, J.S, J.N, J.k);
    PNPP_REQUIRE(J.k <= J.N, PNPP_ERR_RANGE, "selected index k out of range (k=%d > N=%d)", J.k, J.N);
    PNPP_REQUIRE(J.k <= KNN_KMAX, PNPP_ERR_ARG, "knn: nsample=%d exceeds the supported maximum %d", J.k, KNN_KMAX);
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "knn: batch %d exceeds grid limit", B);
    ProfScope ps(st, "knn_kernel B=%d S=%d N=%d k=%d%s", B, J.S, J.N, J.k, J.lengths ? " ragged" : "");
    const auto kfn = J.lengths ? knn_kernel<true> : knn_kernel<false>;
    hipLaunchKernelGGL(kfn, dim3(J.nblocks, B), dim3(256), 0, st, J);
    PNPP_CHECK_LAUNCH("knn");
    return PNPP_OK;
}

int launch_knn(const float *new_xyz, const float *xyz, int B, int S, int N, int k, int32_t *idx, hipStream_t st, const int32_t *lengths) {
    return launch_knn_job({new_xyz, xyz, nullptr, N, S, N, k, idx, nullptr, nullptr, nullptr, nullptr, 1, cdiv(S, 4), lengths, 0}, B, st);
}

// kNN whose queries are gathered centres: also writes the centre coordinates (out_a, optional out_b)
int launch_knn_centres(const float *xyz, const int32_t *centre, int B, int S, int N, int k, int32_t *idx, float *out_a,
                       float *out_b, hipStream_t st, const int32_t *lengths) {
    return launch_knn_job({nullptr, xyz, nullptr, N, S, N, k, idx, centre, out_a, out_b, nullptr, 1, cdiv(S, 4), lengths, 0}, B, st);
}

// queries per wave of level 1 in the pair kernel: two when the cloud is one tile -- a workgroup then stages the cloud once for eight
// queries and writes one moment partial for them (measured at B=32, N=1024, S=128: 16.8 us against 20.6 us with one query per wave,
// and half the partials for the consumer's prologue to read)
static int knn_pair_qpw(int N) { return N <= KNN_TILE ? KNN_PAIR_QPW : 1; }
int knn_pair_moment_partials(int B, int S1, int N) { return B * cdiv(S1, 4 * knn_pair_qpw(N)); }
size_t knn_pair_moment_doubles(int B, int S1, int N) { return (size_t)knn_pair_moment_partials(B, S1, N) * kMomPitch; }

// Both levels' searches in one launch: level 1 = S1 centres (rows centre1 of the N-point cloud), k1 neighbours among the N
// points; level 2 = S2 of those centres (positions centre2 in 0..S1-1), k2 neighbours among the S1 centres.
// mom != nullptr: level 1 also writes knn_pair_moment_partials(B, S1, N) moment partials of its relative coordinates.
int launch_knn_pair(const float *xyz, int B, int N, const int32_t *centre1, int S1, int k1, int32_t *idx1, float *a1, float *b1,
                    const int32_t *centre2, int S2, int k2, int32_t *idx2, float *a2, float *b2, double *mom, hipStream_t st,
                    const int32_t *lengths) {
    PNPP_REQUIRE(xyz && centre1 && centre2 && idx1 && idx2 && a1 && a2, PNPP_ERR_ARG, "knn_pair: null pointer");
    PNPP_REQUIRE(B > 0 && N > 0 && S1 > 0 && S2 > 0 && k1 > 0 && k2 > 0, PNPP_ERR_ARG, "knn_pair: non-positive size");
    PNPP_REQUIRE(k1 <= N && k2 <= S1, PNPP_ERR_RANGE, "selected index k out of range (k=%d > N=%d)", k1 <= N ? k2 : k1, k1 <= N ? S1 : N);
    PNPP_REQUIRE(S1 <= N && S2 <= S1, PNPP_ERR_RANGE, "knn_pair: more centres than points");
    PNPP_REQUIRE(k1 <= KNN_KMAX && k2 <= KNN_KMAX, PNPP_ERR_ARG, "knn: nsample exceeds the supported maximum %d", KNN_KMAX);
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "knn: batch %d exceeds grid limit", B);
    static_assert(KNN_MOM_PITCH == kMomPitch, "moment partial pitch");
    const int qpw = knn_pair_qpw(N), nb1 = cdiv(S1, 4 * qpw), nb2 = cdiv(S2, 4);
    ProfScope ps(st, "knn_pair_kernel B=%d | S=%d N=%d k=%d | S=%d N=%d k=%d%s%s", B, S1, N, k1, S2, S1, k2, mom ? " +moments" : "",
                 lengths ? " ragged" : "");
    const KnnJob J1{nullptr, xyz, nullptr, N, S1, N, k1, idx1, centre1, a1, b1, mom, qpw, nb1, lengths, store_policy()};
    const KnnJob J2{nullptr, xyz, centre1, N, S2, S1, k2, idx2, centre2, a2, b2, nullptr, 1, nb2, nullptr, 0};
    const auto kfn = S1 <= KNN_TILE_SMALL ? (lengths ? knn_pair_kernel<KNN_TILE_SMALL, true> : knn_pair_kernel<KNN_TILE_SMALL, false>)
                                          : (lengths ? knn_pair_kernel<KNN_TILE, true> : knn_pair_kernel<KNN_TILE, false>);
    hipLaunchKernelGGL(kfn, dim3(nb1 + nb2, B), dim3(256), 0, st, J1, J2, nb2);
    PNPP_CHECK_LAUNCH("knn_pair");
    return PNPP_OK;
}

// queries per wave of the normals launch on a cloud of one tile: every point is a query, so a workgroup's 16 KiB of staging serves
// 4 * qpw of them and a wave's one eigen-solve qpw of them.  Measured at 32 x 1024, k = 16 (kernel time): 2: 123.5 us, 4: 105.3 us,
// 8: 96.7 us, 16: 107.7 us (128 workgroups per cloud become 16: too few to fill the CUs).  DESIGN section 17 has the table; the
// macro is there so that a sweep can build the other values (-DKNN_NRM_QPW=n).
#ifndef KNN_NRM_QPW
#define KNN_NRM_QPW 8
#endif

// Normals of all N points of each cloud (include/pnpp_hip.h: pnpp_estimate_normals).  Every refusal comes before the launch.
static int launch_estimate_normals(const float *xyz, int B, int N, int k, int mode, const float *ref, float *out, int stride, float *curv,
                                   int32_t *idx, hipStream_t st, const int32_t *lengths = nullptr) {
    PNPP_REQUIRE(xyz && out, PNPP_ERR_ARG, "estimate_normals: null pointer");
    PNPP_REQUIRE(B > 0 && N > 0, PNPP_ERR_ARG, "estimate_normals: non-positive size (B=%d N=%d)", B, N);
    PNPP_REQUIRE(k >= 3 && k <= KNN_KMAX, PNPP_ERR_ARG, "estimate_normals: k=%d outside the supported range 3..%d", k, KNN_KMAX);
    PNPP_REQUIRE(k <= N, PNPP_ERR_RANGE, "selected index k out of range (k=%d > N=%d)", k, N);
    PNPP_REQUIRE(stride == 3 || stride == 6, PNPP_ERR_ARG, "estimate_normals: output stride %d is neither 3 (normal) nor 6 (xyz, normal)", stride);
    PNPP_REQUIRE(mode == PNPP_NORMALS_NONE || mode == PNPP_NORMALS_AWAY || mode == PNPP_NORMALS_TOWARD, PNPP_ERR_ARG,
                 "estimate_normals: unknown orientation mode %d", mode);
    PNPP_REQUIRE(mode == PNPP_NORMALS_NONE || ref, PNPP_ERR_ARG, "estimate_normals: orientation mode %d needs a reference point per cloud", mode);
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "estimate_normals: batch %d exceeds grid limit", B);
    const int qpw = N <= KNN_TILE ? KNN_NRM_QPW : 1, nb = cdiv(N, 4 * qpw);
    ProfScope ps(st, "knn_normals_kernel B=%d N=%d k=%d%s", B, N, k, lengths ? " ragged" : "");
    const KnnJob J{xyz, xyz, nullptr, N, N, N, k, idx, nullptr, nullptr, nullptr, nullptr, qpw, nb, lengths, 0};
    const KnnNormals W{out, curv, ref, stride, mode};
    const auto kfn = lengths ? knn_normals_kernel<true> : knn_normals_kernel<false>;
    hipLaunchKernelGGL(kfn, dim3(nb, B), dim3(256), 0, st, J, W);
    PNPP_CHECK_LAUNCH("estimate_normals");
    return PNPP_OK;
}

}  // namespace pnpp

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace pnpp;

extern "C" int pnpp_knn(const float *new_xyz, const float *xyz, int B, int S, int N, int k, int32_t *idx, void *stream) {
    return launch_knn(new_xyz, xyz, B, S, N, k, idx, as_stream(stream));
}

extern "C" int pnpp_knn_ragged(const float *new_xyz, const float *xyz, int B, int S, int N, const int32_t *lengths, int k, int32_t *idx,
                               void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "knn_ragged: null lengths");
    return launch_knn(new_xyz, xyz, B, S, N, k, idx, as_stream(stream), lengths);
}

extern "C" int pnpp_estimate_normals(const float *xyz, int B, int N, int k, int orient, const float *ref, float *out, int out_stride,
                                     float *curv, int32_t *idx, void *stream) {
    return launch_estimate_normals(xyz, B, N, k, orient, ref, out, out_stride, curv, idx, as_stream(stream));
}

extern "C" int pnpp_estimate_normals_ragged(const float *xyz, int B, int N, const int32_t *lengths, int k, int orient, const float *ref,
                                            float *out, int out_stride, float *curv, int32_t *idx, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "estimate_normals_ragged: null lengths");
    return launch_estimate_normals(xyz, B, N, k, orient, ref, out, out_stride, curv, idx, as_stream(stream), lengths);
}

extern "C" int pnpp_knn_pair(const float *xyz, int B, int N, const int32_t *centre1, int S1, int k1, int32_t *idx1, float *new_xyz1,
                             const int32_t *centre2, int S2, int k2, int32_t *idx2, float *new_xyz2, double *mom, void *stream) {
    return launch_knn_pair(xyz, B, N, centre1, S1, k1, idx1, new_xyz1, nullptr, centre2, S2, k2, idx2, new_xyz2, nullptr, mom, as_stream(stream));
}
extern "C" int pnpp_knn_pair_ragged(const float *xyz, int B, int N, const int32_t *lengths, const int32_t *centre1, int S1, int k1,
                                    int32_t *idx1, float *new_xyz1, const int32_t *centre2, int S2, int k2, int32_t *idx2,
                                    float *new_xyz2, double *mom, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "knn_pair_ragged: null lengths");
    return launch_knn_pair(xyz, B, N, centre1, S1, k1, idx1, new_xyz1, nullptr, centre2, S2, k2, idx2, new_xyz2, nullptr, mom, as_stream(stream),
                           lengths);
}
extern "C" int pnpp_knn_pair_partials(int B, int S1, int N) {
    return (B > 0 && S1 > 0 && N > 0) ? knn_pair_moment_partials(B, S1, N) : 0;
}
