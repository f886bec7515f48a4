// pointnet_api.hip -- C ABI of the vanilla PointNet kernels (include/pnpp_hip.h, "Vanilla PointNet").  Every argument is checked
// before the first launch.
#include "kernels.h"
#include "pointnet.h"

using namespace pnpp;

namespace {

struct PoolSaved {
    float *mean, *istd, *zsel, *ypre;
    int32_t *route;
    double *S, *Cc;
};

PoolSaved pool_saved_layout(const pnpp_pn_pool_desc *d, void *base, size_t *bytes = nullptr) {
    Carver cv(base);
    const size_t BC = (size_t)d->B * d->C;
    PoolSaved s;
    s.mean = cv.take<float>(d->C);
    s.istd = cv.take<float>(d->C);
    s.zsel = cv.take<float>(BC);
    s.ypre = cv.take<float>(BC);
    s.route = cv.take<int32_t>(BC);
    s.S = cv.take<double>(d->K);
    s.Cc = cv.take<double>((size_t)d->K * d->K);
    if (bytes) *bytes = cv.bytes();
    return s;
}

struct PoolFwdScratch {
    double *gp, *sp;
    float *zmax, *zmin;
    int32_t *imax, *imin;
};

PoolFwdScratch pool_fwd_scratch(const pnpp_pn_pool_desc *d, void *base, size_t *bytes = nullptr) {
    Carver cv(base);
    const size_t BC = (size_t)d->B * d->C;
    PoolFwdScratch s;
    const int ns = pn_gram_slices(d->N);   // per-(cloud, row slice) partials
    s.gp = cv.take<double>((size_t)d->B * ns * d->K * d->K);
    s.sp = cv.take<double>((size_t)d->B * ns * d->K);
    s.zmax = cv.take<float>(BC);
    s.zmin = cv.take<float>(BC);
    s.imax = cv.take<int32_t>(BC);
    s.imin = cv.take<int32_t>(BC);
    if (bytes) *bytes = cv.bytes();
    return s;
}

struct PoolBwdScratch {
    float *coef, *u, *v, *Q, *cvec;
};

PoolBwdScratch pool_bwd_scratch(const pnpp_pn_pool_desc *d, void *base, size_t *bytes = nullptr) {
    Carver cv(base);
    PoolBwdScratch s;
    s.coef = cv.take<float>((size_t)d->B * d->C);
    s.u = cv.take<float>(d->C);
    s.v = cv.take<float>(d->C);
    s.Q = cv.take<float>((size_t)d->K * d->K);
    s.cvec = cv.take<float>(d->K);
    if (bytes) *bytes = cv.bytes();
    return s;
}

// M_total < 0: a uniform batch of B * N rows; otherwise the packed rows of a ragged one
int pool_check(const pnpp_pn_pool_desc *d, long long M_total = -1) {
    PNPP_REQUIRE(d, PNPP_ERR_ARG, "pn_pool: null descriptor");
    PNPP_REQUIRE(d->B > 0 && d->N > 0, PNPP_ERR_ARG, "pn_pool: non-positive size B=%d N=%d", d->B, d->N);
    PNPP_REQUIRE(d->B <= 65535, PNPP_ERR_ARG, "pn_pool: B=%d clouds (at most 65535)", d->B);
    PNPP_REQUIRE(d->K >= 4 && d->K <= 128 && d->K % 4 == 0, PNPP_ERR_ARG, "pn_pool: input width K=%d must be a multiple of 4 in [4, 128]",
                 d->K);
    PNPP_REQUIRE(d->C >= 64 && d->C <= 1024 && d->C % 64 == 0, PNPP_ERR_ARG,
                 "pn_pool: channels C=%d must be a multiple of 64 in [64, 1024]", d->C);
    PNPP_REQUIRE(d->relu == 0 || d->relu == 1, PNPP_ERR_ARG, "pn_pool: relu must be 0 or 1");
    PNPP_REQUIRE(d->training == 0 || d->training == 1, PNPP_ERR_ARG, "pn_pool: training must be 0 or 1");
    PNPP_REQUIRE((long long)d->B * d->N <= (1LL << 31) - 1, PNPP_ERR_ARG, "pn_pool: B*N too large");
    if (M_total >= 0) {
        PNPP_REQUIRE(M_total >= d->B && M_total <= (long long)d->B * d->N, PNPP_ERR_ARG,
                     "pn_pool: M_total=%lld packed rows for B=%d clouds of 1 .. N=%d points", M_total, d->B, d->N);
        if (d->training) PNPP_REQUIRE(M_total > 1, PNPP_ERR_ARG, "Expected more than 1 value per channel when training");
    } else if (d->training) {
        PNPP_REQUIRE((long long)d->B * d->N > 1, PNPP_ERR_ARG, "Expected more than 1 value per channel when training");
    }
    PNPP_REQUIRE(!(d->training && stats_sync_on()), PNPP_ERR_ARG,
                 "pn_pool: the statistics exchange (SyncBN) is registered; the PointNet kernels compute per-process statistics only");
    PNPP_REQUIRE(d->eps > 0.f, PNPP_ERR_ARG, "pn_pool: eps must be positive");
    return PNPP_OK;
}

}  // namespace

#define PN_TRY(x)              \
    do {                       \
        int rc_ = (x);         \
        if (rc_) return rc_;   \
    } while (0)

extern "C" size_t pnpp_pn_pool_saved_bytes(const pnpp_pn_pool_desc *d) {
    if (pool_check(d)) return 0;
    size_t b = 0;
    pool_saved_layout(d, nullptr, &b);
    return b;
}

extern "C" size_t pnpp_pn_pool_scratch_bytes(const pnpp_pn_pool_desc *d) {
    if (pool_check(d)) return 0;
    size_t f = 0, g = 0;
    pool_fwd_scratch(d, nullptr, &f);
    pool_bwd_scratch(d, nullptr, &g);
    return f > g ? f : g;
}

extern "C" void *pnpp_pn_pool_saved_route(const pnpp_pn_pool_desc *d, void *saved) {
    if (pool_check(d) || !saved) return nullptr;
    return pool_saved_layout(d, saved).route;
}

extern "C" void *pnpp_pn_pool_saved_zsel(const pnpp_pn_pool_desc *d, void *saved) {
    if (pool_check(d) || !saved) return nullptr;
    return pool_saved_layout(d, saved).zsel;
}

extern "C" void *pnpp_pn_pool_saved_ypre(const pnpp_pn_pool_desc *d, void *saved) {
    if (pool_check(d) || !saved) return nullptr;
    return pool_saved_layout(d, saved).ypre;
}

static int pool_forward(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_fwd_args *a, const int32_t *offs, long long M, void *stream) {
    PNPP_REQUIRE(a && a->a && a->w && a->b && a->gamma && a->beta && a->rm && a->rv && a->out && a->saved && a->scratch, PNPP_ERR_ARG,
                 "pn_pool_forward: null pointer");
    PNPP_REQUIRE(((uintptr_t)a->a) % 16 == 0, PNPP_ERR_ARG, "pn_pool_forward: the input rows must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    const PoolSaved sv = pool_saved_layout(d, a->saved);
    const PoolFwdScratch sc = pool_fwd_scratch(d, a->scratch);
    if (d->training) PN_TRY(launch_pn_gram(a->a, offs, M, d->B, d->N, d->K, sc.gp, sc.sp, sv.S, sv.Cc, st));
    PN_TRY(launch_pn_pool_scan(a->a, offs, a->w, a->b, d->B, d->N, d->K, d->C, sc.zmax, sc.imax, sc.zmin, sc.imin, st));
    return launch_pn_pool_finalize(a->w, a->b, a->gamma, a->beta, sv.S, sv.Cc, sc.zmax, sc.imax, sc.zmin, sc.imin, d->B, M, d->K,
                                   d->C, d->relu, d->training, d->eps, d->momentum, a->rm, a->rv, (long long *)a->nbt, sv.mean,
                                   sv.istd, sv.zsel, sv.ypre, sv.route, a->out, st);
}

extern "C" int pnpp_pn_pool_forward(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_fwd_args *a, void *stream) {
    PN_TRY(pool_check(d));
    return pool_forward(d, a, nullptr, (long long)d->B * d->N, stream);
}

extern "C" int pnpp_pn_pool_forward_ragged(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_fwd_args *a, const int32_t *offs, int M_total,
                                           void *stream) {
    PN_TRY(pool_check(d, M_total));
    PNPP_REQUIRE(offs, PNPP_ERR_ARG, "pn_pool_forward_ragged: null offsets");
    return pool_forward(d, a, offs, M_total, stream);
}

static int pool_backward(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_bwd_args *a, const int32_t *offs, long long M, void *stream) {
    PNPP_REQUIRE(a && a->a && a->w && a->gamma && a->dout && a->saved && a->scratch && a->dw && a->db && a->dgamma && a->dbeta,
                 PNPP_ERR_ARG, "pn_pool_backward: null pointer");
    hipStream_t st = as_stream(stream);
    const PoolSaved sv = pool_saved_layout(d, const_cast<void *>(a->saved));
    const PoolBwdScratch sc = pool_bwd_scratch(d, a->scratch);
    PN_TRY(launch_pn_pool_bwd_channels(a->a, offs, M, a->w, a->gamma, a->dout, sv.mean, sv.istd, sv.zsel, sv.ypre, sv.route, sv.S, sv.Cc, d->B,
                                       d->N, d->K, d->C, d->relu, d->training, a->dw, a->db, a->dgamma, a->dbeta, sc.coef, sc.u, sc.v,
                                       st));
    if (!a->da) return PNPP_OK;
    if (d->training) PN_TRY(launch_pn_pool_bwd_q(a->w, sc.u, sc.v, d->K, d->C, sc.Q, sc.cvec, st));
    return launch_pn_pool_bwd_da(a->a, offs, M, a->w, sc.Q, sc.cvec, sc.coef, sv.route, sv.S, d->B, d->N, d->K, d->C, d->training, a->da, st);
}

extern "C" int pnpp_pn_pool_backward(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_bwd_args *a, void *stream) {
    PN_TRY(pool_check(d));
    return pool_backward(d, a, nullptr, (long long)d->B * d->N, stream);
}

extern "C" int pnpp_pn_pool_backward_ragged(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_bwd_args *a, const int32_t *offs, int M_total,
                                            void *stream) {
    PN_TRY(pool_check(d, M_total));
    PNPP_REQUIRE(offs, PNPP_ERR_ARG, "pn_pool_backward_ragged: null offsets");
    return pool_backward(d, a, offs, M_total, stream);
}

extern "C" int pnpp_pn_offsets(const int32_t *lengths, int B, int N, int32_t *lens_out, int32_t *offs, void *stream) {
    PNPP_REQUIRE(lengths && lens_out && offs, PNPP_ERR_ARG, "pn_offsets: null pointer");
    PNPP_REQUIRE(B > 0 && N > 0 && B <= 65535, PNPP_ERR_ARG, "pn_offsets: B=%d clouds (1 .. 65535) of N=%d points", B, N);
    PNPP_REQUIRE((long long)B * N <= (1LL << 31) - 1, PNPP_ERR_ARG, "pn_offsets: B*N too large");
    return launch_pn_offsets(lengths, B, N, lens_out, offs, as_stream(stream));
}

// the workspaces of a ragged call have the uniform layout (their sizes follow B, C, K and the padded N's slices, not the row count)
extern "C" size_t pnpp_pn_pool_saved_bytes_ragged(const pnpp_pn_pool_desc *d, int M_total) {
    if (pool_check(d, M_total)) return 0;
    size_t b = 0;
    pool_saved_layout(d, nullptr, &b);
    return b;
}

extern "C" size_t pnpp_pn_pool_scratch_bytes_ragged(const pnpp_pn_pool_desc *d, int M_total) {
    if (pool_check(d, M_total)) return 0;
    size_t f = 0, g = 0;
    pool_fwd_scratch(d, nullptr, &f);
    pool_bwd_scratch(d, nullptr, &g);
    return f > g ? f : g;
}

static int transform_check(const float *x, const float *t, int B, int N, int D, int k, int ldy) {
    PNPP_REQUIRE(x, PNPP_ERR_ARG, "pn_transform: null input");
    PNPP_REQUIRE(B > 0 && N > 0, PNPP_ERR_ARG, "pn_transform: non-positive size B=%d N=%d", B, N);
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "pn_transform: B=%d clouds (at most 65535)", B);
    PNPP_REQUIRE(D >= 1 && D <= 64, PNPP_ERR_ARG, "pn_transform: width D=%d must be in [1, 64]", D);
    PNPP_REQUIRE(ldy >= D && ldy <= 64, PNPP_ERR_ARG, "pn_transform: output width %d must be in [D=%d, 64]", ldy, D);
    if (t) PNPP_REQUIRE(k >= 1 && k <= D, PNPP_ERR_ARG, "pn_transform: transform size k=%d must be in [1, D=%d]", k, D);
    return PNPP_OK;
}

extern "C" int pnpp_pn_transform(const float *x, int64_t sb, int64_t sn, int64_t sd, const float *t, int B, int N, int D, int k, int ldy,
                                 float *y, void *stream) {
    PN_TRY(transform_check(x, t, B, N, D, k, ldy));
    PNPP_REQUIRE(y, PNPP_ERR_ARG, "pn_transform: null output");
    return launch_pn_transform(x, nullptr, 0, sb, sn, sd, t, B, N, D, k, ldy, y, as_stream(stream));
}

extern "C" int pnpp_pn_transform_ragged(const float *x, int x_packed, int64_t sb, int64_t sn, int64_t sd, const float *t, const int32_t *offs,
                                        int B, int N, int D, int k, int ldy, float *y, void *stream) {
    PN_TRY(transform_check(x, t, B, N, D, k, ldy));
    PNPP_REQUIRE(y, PNPP_ERR_ARG, "pn_transform_ragged: null output");
    PNPP_REQUIRE(offs, PNPP_ERR_ARG, "pn_transform_ragged: null offsets");
    return launch_pn_transform(x, offs, x_packed ? 1 : 0, sb, sn, sd, t, B, N, D, k, ldy, y, as_stream(stream));
}

extern "C" int pnpp_pn_transform_bwd(const float *x, int64_t sb, int64_t sn, int64_t sd, const float *t, const float *dy, int B, int N,
                                     int D, int k, int ldy, float *dx, float *dt, void *stream) {
    PN_TRY(transform_check(x, t, B, N, D, k, ldy));
    PNPP_REQUIRE(dy, PNPP_ERR_ARG, "pn_transform_bwd: null output gradient");
    PNPP_REQUIRE(!dt || t, PNPP_ERR_ARG, "pn_transform_bwd: a transform gradient needs the transform");
    return launch_pn_transform_bwd(x, nullptr, 0, sb, sn, sd, t, dy, B, N, D, k, ldy, dx, dt, as_stream(stream));
}

extern "C" int pnpp_pn_transform_bwd_ragged(const float *x, int x_packed, int64_t sb, int64_t sn, int64_t sd, const float *t,
                                            const float *dy, const int32_t *offs, int B, int N, int D, int k, int ldy, float *dx, float *dt,
                                            void *stream) {
    PN_TRY(transform_check(x, t, B, N, D, k, ldy));
    PNPP_REQUIRE(dy, PNPP_ERR_ARG, "pn_transform_bwd_ragged: null output gradient");
    PNPP_REQUIRE(!dt || t, PNPP_ERR_ARG, "pn_transform_bwd_ragged: a transform gradient needs the transform");
    PNPP_REQUIRE(offs, PNPP_ERR_ARG, "pn_transform_bwd_ragged: null offsets");
    return launch_pn_transform_bwd(x, offs, x_packed ? 1 : 0, sb, sn, sd, t, dy, B, N, D, k, ldy, dx, dt, as_stream(stream));
}

extern "C" int pnpp_pn_regularizer(const float *t, int B, int k, double *norms, float *out, void *stream) {
    PNPP_REQUIRE(t && norms && out, PNPP_ERR_ARG, "pn_regularizer: null pointer");
    PNPP_REQUIRE(B > 0 && k >= 1 && k <= 64, PNPP_ERR_ARG, "pn_regularizer: B=%d k=%d (k in [1, 64])", B, k);
    return launch_pn_regularizer(t, B, k, norms, out, as_stream(stream));
}

extern "C" int pnpp_pn_regularizer_bwd(const float *t, const double *norms, const float *dout, int B, int k, float *dt, void *stream) {
    PNPP_REQUIRE(t && norms && dout && dt, PNPP_ERR_ARG, "pn_regularizer_bwd: null pointer");
    PNPP_REQUIRE(B > 0 && k >= 1 && k <= 64, PNPP_ERR_ARG, "pn_regularizer_bwd: B=%d k=%d (k in [1, 64])", B, k);
    return launch_pn_regularizer_bwd(t, norms, dout, B, k, dt, as_stream(stream));
}

extern "C" int pnpp_pn_add_identity(const float *x, int B, int k, float *y, void *stream) {
    PNPP_REQUIRE(x && y, PNPP_ERR_ARG, "pn_add_identity: null pointer");
    PNPP_REQUIRE(B > 0 && k > 0 && (long long)B * k * k < (1LL << 31), PNPP_ERR_ARG, "pn_add_identity: B=%d k=%d", B, k);
    return launch_pn_add_identity(x, B, k, y, as_stream(stream));
}

extern "C" int pnpp_pn_concat(const float *g, const float *pf, int B, int N, int C1, int C2, float *out, void *stream) {
    PNPP_REQUIRE(g && pf && out, PNPP_ERR_ARG, "pn_concat: null pointer");
    PNPP_REQUIRE(B > 0 && N > 0 && C1 > 0 && C2 > 0, PNPP_ERR_ARG, "pn_concat: non-positive size");
    return launch_pn_concat(g, pf, nullptr, 0, B, N, C1, C2, out, as_stream(stream));
}

extern "C" int pnpp_pn_concat_ragged(const float *g, const float *pf, int pf_padded, const int32_t *offs, int B, int N, int C1, int C2,
                                     float *out, void *stream) {
    PNPP_REQUIRE(g && pf && out, PNPP_ERR_ARG, "pn_concat_ragged: null pointer");
    PNPP_REQUIRE(offs, PNPP_ERR_ARG, "pn_concat_ragged: null offsets");
    PNPP_REQUIRE(B > 0 && N > 0 && C1 > 0 && C2 > 0, PNPP_ERR_ARG, "pn_concat_ragged: non-positive size");
    return launch_pn_concat(g, pf, offs, pf_padded ? 1 : 0, B, N, C1, C2, out, as_stream(stream));
}

extern "C" int pnpp_pn_concat_bwd(const float *dout, int B, int N, int C1, int C2, float *dg, float *dpf, void *stream) {
    PNPP_REQUIRE(dout, PNPP_ERR_ARG, "pn_concat_bwd: null output gradient");
    PNPP_REQUIRE(B > 0 && N > 0 && C1 > 0 && C2 > 0, PNPP_ERR_ARG, "pn_concat_bwd: non-positive size");
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "pn_concat_bwd: B=%d clouds (at most 65535)", B);
    return launch_pn_concat_bwd(dout, nullptr, B, N, C1, C2, dg, dpf, as_stream(stream));
}

extern "C" int pnpp_pn_concat_bwd_ragged(const float *dout, const int32_t *offs, int B, int N, int C1, int C2, float *dg, float *dpf,
                                         void *stream) {
    PNPP_REQUIRE(dout, PNPP_ERR_ARG, "pn_concat_bwd_ragged: null output gradient");
    PNPP_REQUIRE(offs, PNPP_ERR_ARG, "pn_concat_bwd_ragged: null offsets");
    PNPP_REQUIRE(B > 0 && N > 0 && C1 > 0 && C2 > 0, PNPP_ERR_ARG, "pn_concat_bwd_ragged: non-positive size");
    PNPP_REQUIRE(B <= 65535, PNPP_ERR_ARG, "pn_concat_bwd_ragged: B=%d clouds (at most 65535)", B);
    return launch_pn_concat_bwd(dout, offs, B, N, C1, C2, dg, dpf, as_stream(stream));
}

extern "C" int pnpp_pn_bn_relu(const float *x, int M, int C, const float *gamma, const float *beta, float *rm, float *rv, int64_t *nbt,
                               int training, float eps, float momentum, float *mean, float *istd, float *y, void *stream) {
    PNPP_REQUIRE(x && gamma && beta && rm && rv && mean && istd && y, PNPP_ERR_ARG, "pn_bn_relu: null pointer");
    PNPP_REQUIRE(M > 0 && C > 0, PNPP_ERR_ARG, "pn_bn_relu: non-positive size M=%d C=%d", M, C);
    if (training) PNPP_REQUIRE(M > 1, PNPP_ERR_ARG, "Expected more than 1 value per channel when training");
    PNPP_REQUIRE(!(training && stats_sync_on()), PNPP_ERR_ARG,
                 "pn_bn_relu: the statistics exchange (SyncBN) is registered; the PointNet kernels compute per-process statistics only");
    return launch_pn_bn_relu(x, M, C, gamma, beta, rm, rv, (long long *)nbt, training, eps, momentum, mean, istd, y, as_stream(stream));
}

extern "C" int pnpp_pn_bn_relu_bwd(const float *x, const float *y, const float *dy, int M, int C, const float *gamma, const float *mean,
                                   const float *istd, int training, float *dx, float *dgamma, float *dbeta, void *stream) {
    PNPP_REQUIRE(x && y && dy && gamma && mean && istd && dgamma && dbeta, PNPP_ERR_ARG, "pn_bn_relu_bwd: null pointer");
    PNPP_REQUIRE(M > 0 && C > 0, PNPP_ERR_ARG, "pn_bn_relu_bwd: non-positive size M=%d C=%d", M, C);
    return launch_pn_bn_relu_bwd(x, y, dy, M, C, gamma, mean, istd, training, dx, dgamma, dbeta, as_stream(stream));
}
