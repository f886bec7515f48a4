// fc_api.hip -- host side of the fully connected block Linear -> {BatchNorm1d | LayerNorm | none} -> ReLU -> dropout: the
// workspace layouts, the argument requirements and which launches a call takes.  The block's own kernels and their launchers are
// csrc/fc_kernels.hip (csrc/fc.h); the matrix products run on the fused MFMA GEMM / dW kernels of the set-abstraction layers.
//
// One FcBlock is built per call; its routing facts, each decided once from the descriptor (and the process-wide statistics
// exchange), select the steps:
//   forward
//     1. `small`: fc_small_fwd_kernel, which ends the pass;
//     2. fc_fwd_product: the product into the kept z -- `one_tile_bn`: with the E_BN_APPLY epilogue (statistics, affine, ReLU,
//        dropout in the GEMM), which ends the pass; training BatchNorm: with column statistics; otherwise a plain store;
//     3. fc_fwd_apply: BatchNorm: (exchange,) bn_finalize_fwd_kernel, fc_apply_cols_kernel; LayerNorm: fc_apply_ln_kernel;
//        none: fc_apply_cols_kernel.
//   backward
//     1. `small`: fc_small_bwd_kernel, which ends the pass;
//     2. `fused_bwd`: fc_bwd_fused (fc_bwd_fused_kernel: dx, dW and the parameter gradients, dz never written), which ends the pass;
//     3. fc_bwd_dz, one of: LayerNorm: fc_bwd_ln_rows_kernel + fc_bwd_ln_cols_kernel; none and `row_chunked`: fc_bwd_rows_kernel +
//        slab_reduce_kernel; BatchNorm, `row_chunked`, no exchange: fc_bwd_bn_rows_sums_kernel + fc_bwd_bn_rows_apply_kernel;
//        `sync_bn`: fc_bwd_cols_kernel phase 1, the exchange, phase 2; otherwise one fc_bwd_cols_kernel launch (phase 0);
//     4. fc_bwd_dw, one of: a gradient to pass on and fc_dx_dw_kernel takes the shape (try_launch_fc_dx_dw), which ends the
//        pass; M <= 32: dw_fewrows_kernel; one partial in dW's own layout: dw_kernel in place; otherwise dw_kernel +
//        slab_reduce_kernel;
//     5. fc_bwd_dx: dx = dz W, if wanted.
#include "fc.h"
#include "launch.h"

namespace pnpp {

struct FcSaved {
    float *z, *mean, *istd, *scale, *shift;
    size_t bytes;
};
static FcSaved fc_saved_layout(const pnpp_fc_desc *d, void *base) {
    Carver cv(base);
    FcSaved s;
    const int mx = d->M > d->N ? d->M : d->N;
    s.z = cv.take<float>((size_t)d->M * d->N);
    s.mean = cv.take<float>(mx);
    s.istd = cv.take<float>(mx);
    s.scale = cv.take<float>(d->N);
    s.shift = cv.take<float>(d->N);
    s.bytes = cv.bytes();
    return s;
}
struct FcScratch {
    float *dz, *gbuf, *dwslab;
    double *slab;
    size_t bytes;
};
static FcScratch fc_scratch_layout(const pnpp_fc_desc *d, void *base) {
    Carver cv(base);
    FcScratch s;
    s.slab = cv.take<double>((size_t)kMaxStatBlocks * 2 * d->N);
    s.dz = cv.take<float>((size_t)d->M * d->N);
    s.gbuf = cv.take<float>((size_t)d->M * d->N);
    int nsplit, kp_pad;
    dw_plan(d->M, d->N, d->K, &nsplit, &kp_pad);
    s.dwslab = cv.take<float>((size_t)nsplit * d->N * kp_pad);
    s.bytes = cv.bytes();
    return s;
}

static bool fc_is_small(const pnpp_fc_desc *d) { return d->norm == PNPP_NORM_NONE && d->N <= FC_SMALL_N; }

static int fc_check(const pnpp_fc_desc *d) {
    PNPP_REQUIRE(d, PNPP_ERR_ARG, "fc: null descriptor");
    PNPP_REQUIRE(d->M > 0 && d->K > 0 && d->N > 0, PNPP_ERR_ARG, "fc: non-positive size M=%d K=%d N=%d", d->M, d->K, d->N);
    if (!fc_is_small(d))
        PNPP_REQUIRE(d->K % 4 == 0 && d->N % 4 == 0, PNPP_ERR_ARG, "fc: K=%d and N=%d must be multiples of 4", d->K, d->N);
    PNPP_REQUIRE(d->norm >= PNPP_NORM_NONE && d->norm <= PNPP_NORM_LAYER, PNPP_ERR_ARG, "fc: bad norm kind %d", d->norm);
    return PNPP_OK;
}

// ---- one call's view of a block, built once on the stack: the descriptor, the routing facts, the two workspaces ----
struct FcBlock {
    const pnpp_fc_desc *d = nullptr;
    hipStream_t st = nullptr;
    bool bn = false;            // BatchNorm1d
    bool exchange = false;      // the statistics exchange over the ranks is registered (SyncBN)
    // the routing facts
    bool small = false;         // no normalisation, N <= FC_SMALL_N: the dot-product kernels
    bool one_tile_bn = false;   // training BatchNorm, M <= 32, no exchange: the whole batch is one tile, the GEMM epilogue finishes the block
    bool row_chunked = false;   // M > 4096: the backward reductions over the rows are split into 256-row chunks
    bool fused_bwd = false;     // M <= 32 with a gradient to pass on: one backward launch, dz never written (PNPP_NO_FC_FUSED=1 keeps the two launches)
    bool sync_bn = false;       // training BatchNorm with the exchange: the backward sums cross the ranks between two phases
    FcSaved sv;
    FcScratch sc;

    AOperand plain(const float *a, int lda) const {
        AOperand A;
        A.mode = A_PLAIN, A.a = a, A.lda = lda;
        return A;
    }
    FcGrad grad(const pnpp_fc_bwd_args *a) const {
        return FcGrad{a->dy, sv.z, a->mask, d->drop_scale, d->relu, bn, d->training, sv.scale, sv.shift, sv.mean, sv.istd, a->b, d->M, d->N};
    }
};

static FcBlock fc_block_plan(const pnpp_fc_desc *d, void *saved, void *scratch, bool want_dx, hipStream_t st) {
    FcBlock F;
    F.d = d, F.st = st;
    F.bn = d->norm == PNPP_NORM_BATCH;
    F.exchange = stats_sync_on();
    F.small = fc_is_small(d);
    F.one_tile_bn = F.bn && d->training && d->M <= 32 && !F.exchange;
    F.row_chunked = d->M > 4096;
    F.sync_bn = F.bn && d->training && F.exchange;
    static const bool fused_on = env_int("PNPP_NO_FC_FUSED", 0) == 0;
    F.fused_bwd = fused_on && want_dx && d->norm != PNPP_NORM_LAYER && d->M <= 32 && d->N >= 256 && d->N % 2 == 0 && !F.sync_bn &&
                  fc_bwd_fused_lds(d->N) <= 160 * 1024;
    F.sv = fc_saved_layout(d, saved);
    F.sc = fc_scratch_layout(d, scratch);
    return F;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
static FcDraw fc_draw(const pnpp_fc_fwd_args *a) {
    FcDraw D;
    D.mask_out = a->mask_out, D.drop_p = a->drop_p, D.rng_seed = (unsigned long long)a->rng_seed;
    D.rng_counter = reinterpret_cast<unsigned long long *>(a->rng_counter);
    return D;
}

// z = x W^T into the kept workspace.  one_tile_bn: the epilogue finishes the block (y, the statistics kept for backward, the running
// statistics, the drawn mask); training BatchNorm: + column statistics (*nslab slabs)
static int fc_fwd_product(const FcBlock &F, const pnpp_fc_fwd_args *a, int *nslab) {
    const pnpp_fc_desc *d = F.d;
    BOperand W;  // the linear weight (N x K) is read in place
    W.b = a->w, W.ldb = d->K, W.trans = 1, W.rows = d->K;
    const AOperand A = F.plain(a->x, d->K);
    Epilogue E;
    E.c = F.sv.z, E.ldc = d->N;
    if (F.one_tile_bn) {
        E.mode = E_BN_APPLY;
        BnTail &T = E.bn;
        T.bias = a->b, T.gamma = a->nw, T.beta = a->nb;
        T.rm = a->rm, T.rv = a->rv, T.nbt = (long long *)a->nbt;
        T.momentum = d->momentum, T.eps = d->eps;
        T.mean = F.sv.mean, T.istd = F.sv.istd, T.scale = F.sv.scale, T.shift = F.sv.shift;
        T.mask = a->mask, T.drop_scale = d->drop_scale, T.relu = d->relu, T.y = a->y;
        if (a->mask_out) {
            const FcDraw D = fc_draw(a);
            T.mask_out = D.mask_out, T.drop_p = D.drop_p, T.rng_seed = D.rng_seed, T.rng_counter = D.rng_counter;
        }
        return launch_gemm(A, W, d->M, d->N, d->K, E, nullptr, F.st);
    }
    if (F.bn && d->training) {
        E.mode = E_STORE_STATS;
        E.slab = F.sc.slab;
        return launch_gemm(A, W, d->M, d->N, d->K, E, nslab, F.st);
    }
    E.mode = E_STORE;
    return launch_gemm(A, W, d->M, d->N, d->K, E, nullptr, F.st);
}

// y from z: the normalisation (BatchNorm: its finalisation first), ReLU, dropout
static int fc_fwd_apply(const FcBlock &F, const pnpp_fc_fwd_args *a, int nslab) {
    const pnpp_fc_desc *d = F.d;
    const FcSaved &sv = F.sv;
    if (d->norm == PNPP_NORM_LAYER)
        return launch_fc_apply_ln(sv.z, a->b, a->nw, a->nb, a->mask, d->drop_scale, d->relu, d->M, d->N, d->eps, a->y, sv.mean, sv.istd,
                                  fc_draw(a), F.st);
    if (!F.bn)
        return launch_fc_apply_cols(sv.z, (const float *)nullptr, a->b, a->mask, d->drop_scale, d->relu, d->M, d->N, a->y, true, "fc_forward",
                                    F.st);
    StatsView V;
    V.slab = F.sc.slab, V.nslab = nslab;
    if (d->training) PNPP_TRY(stats_exchange(F.sc.slab, nslab, d->N, (double)d->M, F.st, &V));
    BnLayer bn;
    bn.C = d->N, bn.bias = a->b, bn.gamma = a->nw, bn.beta = a->nb, bn.rm = a->rm, bn.rv = a->rv, bn.nbt = (long long *)a->nbt;
    bn.mean = sv.mean, bn.istd = sv.istd, bn.scale = sv.scale, bn.shift = sv.shift;
    PNPP_TRY(launch_bn_finalize_fwd(V, (double)d->M, bn, BnHyper{d->momentum, d->eps, d->training}, F.st));
    return launch_fc_apply_cols(sv.z, sv.scale, sv.shift, a->mask, d->drop_scale, d->relu, d->M, d->N, a->y, false, "fc_forward", F.st);
}

static int fc_forward_impl(const pnpp_fc_desc *d, const pnpp_fc_fwd_args *a, hipStream_t st) {
    PNPP_TRY(fc_check(d));
    PNPP_REQUIRE(a && a->x && a->w && a->b && a->y && a->saved && a->scratch, PNPP_ERR_ARG, "fc_forward: null pointer");
    if (d->norm != PNPP_NORM_NONE) PNPP_REQUIRE(a->nw && a->nb, PNPP_ERR_ARG, "fc_forward: norm affine parameters are null");
    if (d->norm == PNPP_NORM_BATCH) PNPP_REQUIRE(a->rm && a->rv, PNPP_ERR_ARG, "fc_forward: running statistics are null");
    const FcBlock F = fc_block_plan(d, a->saved, a->scratch, false, st);
    PNPP_REQUIRE(!a->mask_out || F.one_tile_bn || (d->training && d->norm == PNPP_NORM_LAYER), PNPP_ERR_ARG,
                 "fc_forward: the in-kernel dropout draw exists for the BatchNorm epilogue (training, M <= 32, no statistics "
                 "exchange) and for the LayerNorm block (training) only");
    if (a->mask_out)
        PNPP_REQUIRE(!a->mask && a->rng_counter && a->drop_p > 0.f && a->drop_p < 1.f, PNPP_ERR_ARG,
                     "fc_forward: a drawn dropout mask needs rng_counter, 0 < drop_p < 1 and no given mask");
    if (F.small) return launch_fc_small_fwd(a->x, a->w, a->b, a->mask, d->drop_scale, d->relu, d->M, d->K, d->N, F.sv.z, a->y, st);
    if (F.bn && d->training) PNPP_REQUIRE(d->M > 1, PNPP_ERR_ARG, "Expected more than 1 value per channel when training");  // torch's message
    int nslab = 0;
    PNPP_TRY(fc_fwd_product(F, a, &nslab));
    if (F.one_tile_bn) return PNPP_OK;
    return fc_fwd_apply(F, a, nslab);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
static BnGrads fc_param_grads(const pnpp_fc_bwd_args *a) { return BnGrads{a->dnw, a->dnb, a->db}; }

// dz = d loss / d (x W^T)  (M x N) into the scratch workspace, and the parameter gradients of the normalisation
static int fc_bwd_dz(const FcBlock &F, const pnpp_fc_bwd_args *a) {
    const pnpp_fc_desc *d = F.d;
    const FcScratch &sc = F.sc;
    const FcGrad g = F.grad(a);
    const BnGrads pg = fc_param_grads(a);
    if (d->norm == PNPP_NORM_LAYER) {
        PNPP_TRY(launch_fc_bwd_ln_rows(g, a->nw, a->nb, sc.dz, sc.gbuf, F.st));
        return launch_fc_bwd_ln_cols(g, sc.gbuf, sc.dz, pg, F.st);
    }
    if (!F.bn && F.row_chunked) {   // sc.gbuf (M x N floats) holds the [chunks][N] partials
        PNPP_TRY(launch_fc_bwd_rows(g, sc.dz, sc.gbuf, F.st));
        return launch_slab_reduce(sc.gbuf, fc_row_chunks(d->M), 1, d->N, d->N, -1, a->db, d->N, F.st);
    }
    if (F.bn && F.row_chunked && !F.exchange) {   // sc.gbuf (M x N floats) holds the [chunks][2N] float64 partials
        double *part = reinterpret_cast<double *>(sc.gbuf);
        PNPP_TRY(launch_fc_bwd_bn_rows_sums(g, part, F.st));
        return launch_fc_bwd_bn_rows_apply(g, part, sc.dz, pg, F.st);
    }
    if (F.sync_bn) {   // SyncBN: sums -> exchange over the ranks -> apply
        PNPP_TRY(launch_fc_bwd_cols(g, sc.dz, pg, 1, stats_buffer_global(), stats_buffer_local(), F.st));
        StatsView V;
        PNPP_TRY(stats_exchange_inplace(d->N, F.st, &V));
        return launch_fc_bwd_cols(g, sc.dz, pg, 2, stats_buffer_global(), stats_buffer_local(), F.st);
    }
    return launch_fc_bwd_cols(g, sc.dz, pg, 0, (double *)nullptr, (double *)nullptr, F.st);
}

// dW = dz^T x.  *done: the launch also wrote dx = dz W (head layers with a gradient to pass on), the pass is over
static int fc_bwd_dw(const FcBlock &F, const pnpp_fc_bwd_args *a, bool *done) {
    const pnpp_fc_desc *d = F.d;
    const FcScratch &sc = F.sc;
    int rc = PNPP_OK;
    *done = a->dx && try_launch_fc_dx_dw(sc.dz, a->w, a->x, d->M, d->N, d->K, a->dx, a->dw, F.st, &rc);
    if (*done) return rc;
    if (d->M <= 32) return launch_dw_fewrows(sc.dz, a->x, d->M, d->N, d->K, a->dw, F.st);   // a handful of rows: outer-product kernel, written in place
    const AOperand dz = F.plain(sc.dz, d->N), x = F.plain(a->x, d->K);
    int nsplit, kp_pad;
    dw_plan(d->M, d->N, d->K, &nsplit, &kp_pad);
    if (nsplit == 1 && kp_pad == d->K)   // a single partial in the gradient's own layout: write it in place
        return launch_dw(dz, d->N, x, d->K, d->M, a->dw, 1, kp_pad, F.st);
    PNPP_TRY(launch_dw(dz, d->N, x, d->K, d->M, sc.dwslab, nsplit, kp_pad, F.st));
    return launch_slab_reduce(sc.dwslab, nsplit, d->N, kp_pad, d->K, -1, a->dw, d->K, F.st);
}

// dx = dz W
static int fc_bwd_dx(const FcBlock &F, const pnpp_fc_bwd_args *a) {
    const pnpp_fc_desc *d = F.d;
    if (!a->dx) return PNPP_OK;
    Epilogue E;
    E.mode = E_STORE, E.c = a->dx, E.ldc = d->K;
    BOperand W;
    W.b = a->w, W.ldb = d->K, W.rows = d->N;
    return launch_gemm(F.plain(F.sc.dz, d->N), W, d->M, d->K, d->N, E, nullptr, F.st);
}

static int fc_bwd_fused(const FcBlock &F, const pnpp_fc_bwd_args *a) {
    return launch_fc_bwd_fused(F.grad(a), a->w, a->x, F.d->K, a->dx, a->dw, fc_param_grads(a), F.st);
}

static int fc_backward_impl(const pnpp_fc_desc *d, const pnpp_fc_bwd_args *a, hipStream_t st) {
    PNPP_TRY(fc_check(d));
    PNPP_REQUIRE(a && a->x && a->w && a->b && a->dy && a->saved && a->scratch && a->dw && a->db, PNPP_ERR_ARG,
                 "fc_backward: null pointer");
    if (d->norm != PNPP_NORM_NONE) PNPP_REQUIRE(a->nw && a->nb, PNPP_ERR_ARG, "fc_backward: norm affine parameters are null");
    const FcBlock F = fc_block_plan(d, const_cast<void *>(a->saved), a->scratch, a->dx != nullptr, st);
    if (F.small) return launch_fc_small_bwd(F.grad(a), a->x, a->w, d->K, a->dw, a->db, a->dx, st);
    if (F.fused_bwd) return fc_bwd_fused(F, a);
    PNPP_TRY(fc_bwd_dz(F, a));
    bool done = false;
    PNPP_TRY(fc_bwd_dw(F, a, &done));
    return done ? PNPP_OK : fc_bwd_dx(F, a);
}

}  // namespace pnpp

using namespace pnpp;

extern "C" size_t pnpp_fc_saved_bytes(const pnpp_fc_desc *d) { return fc_check(d) == PNPP_OK ? fc_saved_layout(d, nullptr).bytes : 0; }
extern "C" size_t pnpp_fc_scratch_bytes(const pnpp_fc_desc *d) {
    return fc_check(d) == PNPP_OK ? fc_scratch_layout(d, nullptr).bytes : 0;
}
extern "C" int pnpp_fc_forward(const pnpp_fc_desc *d, const pnpp_fc_fwd_args *a, void *stream) {
    return fc_forward_impl(d, a, as_stream(stream));
}
extern "C" int pnpp_fc_backward(const pnpp_fc_desc *d, const pnpp_fc_bwd_args *a, void *stream) {
    return fc_backward_impl(d, a, as_stream(stream));
}
// y of a BatchNorm block with more than 32 rows, recomputed from what its forward call kept (the same launcher as the forward pass's
// last launch, so the same bits): lets a caller drop y between forward and backward (models/pointnet.py's per-point trunks)
extern "C" int pnpp_fc_recompute_output(const pnpp_fc_desc *d, const void *saved, const uint8_t *mask, float *y, void *stream) {
    PNPP_TRY(fc_check(d));
    PNPP_REQUIRE(saved && y, PNPP_ERR_ARG, "fc_recompute_output: null pointer");
    PNPP_REQUIRE(d->norm == PNPP_NORM_BATCH && d->M > 32, PNPP_ERR_ARG,
                 "fc_recompute_output: only BatchNorm blocks with more than 32 rows (M=%d norm=%d)", d->M, d->norm);
    const FcSaved sv = fc_saved_layout(d, const_cast<void *>(saved));
    return launch_fc_apply_cols(sv.z, sv.scale, sv.shift, mask, d->drop_scale, d->relu, d->M, d->N, y, true, "fc_recompute_output",
                                as_stream(stream));
}
