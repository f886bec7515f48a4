// sa_api.hip -- host-side orchestration of PointNetSetAbstraction forward / backward on top of the fused kernels
// (gemm_*_kernels.hip, knn_kernels.hip, sampling_kernels.hip, group_kernels.hip).  The library's runtime -- errors, launch timing, the SyncBN exchange -- is runtime.hip.
// Reference: models/pointnet_pp_8dir.py:21-43 (forward) and its autograd graph.
//
// Everything is stream-ordered: these functions only enqueue work on `stream`; they never allocate,
// free, copy to the host or synchronise (they can be captured into a hipGraph).
#include "launch.h"

namespace pnpp {

struct SaGeom {
    int M, G, maxC;
    int Cin[PNPP_MAX_LAYERS];  // reduction dim of layer l in state_dict terms (D+3 for l = 0)
    int Kd[PNPP_MAX_LAYERS];   // padded reduction dim used by the kernels
};

static int sa_geom(const pnpp_sa_desc *d, SaGeom *g) {
    PNPP_REQUIRE(d, PNPP_ERR_ARG, "sa: null descriptor");
    PNPP_REQUIRE(d->B > 0 && d->N > 0 && d->S > 0 && d->K > 0 && d->D >= 0, PNPP_ERR_ARG,
                 "sa: bad geometry B=%d N=%d S=%d K=%d D=%d", d->B, d->N, d->S, d->K, d->D);
    PNPP_REQUIRE(d->L >= 1 && d->L <= PNPP_MAX_LAYERS, PNPP_ERR_ARG, "sa: unsupported layer count %d", d->L);
    if (d->group_all) PNPP_REQUIRE(d->S == 1 && d->K == d->N, PNPP_ERR_ARG, "sa: group_all needs S == 1 and K == N");
    PNPP_REQUIRE((long long)d->B * d->S * d->K < (1ll << 31), PNPP_ERR_ARG, "sa: B*S*K overflows int32");
    g->M = d->B * d->S * d->K;
    g->G = d->B * d->S;
    g->maxC = 0;
    for (int l = 0; l < d->L; ++l) {
        PNPP_REQUIRE(d->C[l] > 0 && d->C[l] % 32 == 0, PNPP_ERR_ARG,
                     "sa: mlp channel %d (=%d) must be a positive multiple of 32 for the MFMA path", l, d->C[l]);
        g->maxC = d->C[l] > g->maxC ? d->C[l] : g->maxC;
        g->Cin[l] = l == 0 ? d->D + 3 : d->C[l - 1];
        g->Kd[l] = l == 0 ? (d->D + 3 + 3) & ~3 : d->C[l - 1];
    }
    return PNPP_OK;
}

struct SaSaved {
    int32_t *idx;
    float *new_xyz;
    float *z[PNPP_MAX_LAYERS];
    float *mean[PNPP_MAX_LAYERS], *istd[PNPP_MAX_LAYERS], *scale[PNPP_MAX_LAYERS], *shift[PNPP_MAX_LAYERS];
    int32_t *arg;
    double *mom;   // a level on raw coordinates grouped by pnpp_sa_group_pair: the moment partials its search wrote (SaLevel::pair_moments)
    float *zmax;   // (G, C_last): the pre-BN value each pooled output came from (the backward pass's ReLU gate and xhat need it)
    size_t bytes;
};

struct SaScratch {
    double *slab;
    float *dy[2];
    float *dzbuf;  // small-M layers only: materialised dZ
    float *dm;
    float *cst;    // the BatchNorm-backward constants of the layer being processed (written by the finalisation that precedes it)
    float *dwslab;
    float *src;  // convolve-then-gather layer 0: one C_0-wide row per source point (P forward, G backward)
    float *xslab;  // ... and the [C_0][4] dW_xyz partials of its backward scatter
    double *mom;   // a level on raw coordinates: moment partials of the relative coordinates (gemm_wsx_kernels.hip)
    size_t bytes;
};

constexpr int kSmallM = 4096;  // at or below this many rows dZ is materialised once per layer (group_all layers)
static Epilogue store_to(float *c, int ldc) {
    Epilogue E;
    E.mode = E_STORE, E.c = c, E.ldc = ldc;
    return E;
}

// ---- one call's view of a level, built once on the stack: geometry, routing facts, workspaces, the layers as values ----
struct SaLevel {
    const pnpp_sa_desc *d = nullptr;
    hipStream_t st = nullptr;
    SaGeom g;
    // the routing facts: functions of the geometry (and the process-wide modes) alone, so both passes, the size queries and the pair search agree
    bool xyz0 = false;          // on raw coordinates (SA1): no Z_0 -- statistics from the coordinate moments, layer 1 builds its operand (gemm_wsx_kernels.hip)
    bool delayed = false;       // layer 0 is convolved on the B*N source points and gathered afterwards (a level grouping points WITH features)
    bool keeps_zmax = false;    // false: whole-cloud pooling in K chunks (pool_fwd_split / merge) produces no selected pre-BN values
    bool small = false;         // M <= kSmallM: dZ is materialised once per layer, in the launch that finalises the layer's sums
    bool pair_moments = false;  // the pair search also sums this level's coordinate moments into sv.mom: no rel_moments launch then
    SaSaved sv;
    SaScratch sc;
    const float *xyz = nullptr, *points = nullptr;
    const float *const *conv_w = nullptr;
    BnLayer bn[PNPP_MAX_LAYERS];    // gamma always; bias / beta / running statistics in a forward call
    BnGrads dbn[PNPP_MAX_LAYERS];   // backward calls
    BnHyper hyper;
    bool want_dpoints = false;      // backward calls
    const SaTail *ride = nullptr;   // backward calls: a reduction deferred by the level above, run behind this level's opening launch
    SaTail *defer = nullptr;        // backward calls: where the level's last reduction is described instead of launched

    double count() const { return (double)g.M; }
    AOperand layer0_operand() const {
        AOperand A;
        A.mode = d->group_all ? A_CONCAT : A_GATHER;
        A.a = points, A.xyz = xyz, A.new_xyz = sv.new_xyz, A.idx = sv.idx;
        A.D = d->D, A.N = d->N, A.S = d->S, A.K = d->K;
        return A;
    }
    AOperand input_of(int l) const {   // what layer l multiplies: the grouped input, or relu(bn(Z_{l-1})) applied by the operand loader
        if (l == 0) return layer0_operand();
        AOperand A;
        A.mode = A_BNRELU;
        A.a = sv.z[l - 1], A.lda = d->C[l - 1], A.scale = sv.scale[l - 1], A.shift = sv.shift[l - 1];
        return A;
    }
    BOperand weight(int l, int rows) const {   // W_l (C_l x Cin_l) row-major as stored, `rows` valid reduction rows
        BOperand W;
        W.b = conv_w[l], W.ldb = g.Cin[l], W.rows = rows;
        return W;
    }
    BOperand w0_features() const {   // feature columns of W_0: (C_0 x (3+D)) row-major, skip the three xyz columns
        BOperand W = weight(0, d->C[0]);
        W.b += 3;
        return W;
    }
    // dZ_l as the kernels rebuild it; the top layer's dense gradient is never materialised (A_DZ_POOL rebuilds it from dm / arg)
    AOperand dz_operand(int l, int buf) const {
        const bool top = l == d->L - 1;
        AOperand dz;
        dz.mode = top ? A_DZ_POOL : A_DZ, dz.a = top ? sc.dm : sc.dy[buf];
        dz.arg = sv.arg, dz.K = d->K, dz.lda = dz.C = d->C[l], dz.z = sv.z[l], dz.cst = sc.cst;
        return dz;
    }
    DzSide dz_side(const AOperand *dz) const { return small ? DzSide{dz, g.M, sc.dzbuf} : DzSide(); }
};

static int sa_level_plan(const pnpp_sa_desc *d, SaLevel *L) {
    PNPP_TRY(sa_geom(d, &L->g));
    const SaGeom &g = L->g;
    L->d = d;
    L->xyz0 = xyz0_applies(g.M, d->D, d->K, d->group_all, d->L, d->C);
    L->delayed = !d->group_all && d->D > 0 && d->D % 4 == 0 && delayed_layer0_ok(d->C[0]) && d->S * d->K > d->N;
    L->keeps_zmax = pool_fwd_splits(g.G, d->K, d->C[d->L - 1]) <= 1;
    L->small = g.M <= kSmallM;
    L->pair_moments = L->xyz0;
    return PNPP_OK;
}

static SaSaved sa_saved_layout(const SaLevel &L, void *base) {
    const pnpp_sa_desc *d = L.d;
    const SaGeom &g = L.g;
    Carver cv(base);
    SaSaved s;
    s.idx = cv.take<int32_t>(d->group_all ? 0 : (size_t)g.M);
    s.new_xyz = cv.take<float>((size_t)g.G * 3);
    for (int l = 0; l < d->L; ++l) {
        s.z[l] = cv.take<float>((size_t)g.M * d->C[l]);
        s.mean[l] = cv.take<float>(d->C[l]);
        s.istd[l] = cv.take<float>(d->C[l]);
        s.scale[l] = cv.take<float>(d->C[l]);
        s.shift[l] = cv.take<float>(d->C[l]);
    }
    s.arg = cv.take<int32_t>((size_t)g.G * d->C[d->L - 1]);
    s.zmax = cv.take<float>(L.keeps_zmax ? (size_t)g.G * d->C[d->L - 1] : 0);
    s.mom = cv.take<double>(L.pair_moments ? knn_pair_moment_doubles(d->B, d->S, d->N) : 0);
    s.bytes = cv.bytes();
    return s;
}

static SaScratch sa_scratch_layout(const SaLevel &L, void *base) {
    const pnpp_sa_desc *d = L.d;
    const SaGeom &g = L.g;
    Carver cv(base);
    SaScratch s;
    {   // BatchNorm partial sums of one layer; a level on raw coordinates also parks layer 0's backward sums here (gemm_wsx_kernels.hip)
        size_t nd = (size_t)kMaxStatBlocks * 2 * g.maxC;
        if (!d->group_all && d->D == 0 && wsx_stat_doubles() > nd) nd = wsx_stat_doubles();
        s.slab = cv.take<double>(nd);
    }
    const int wide = g.maxC > d->D ? g.maxC : d->D;
    s.dy[0] = cv.take<float>((size_t)g.M * wide);
    s.dy[1] = cv.take<float>((size_t)g.M * wide);
    s.dzbuf = cv.take<float>(L.small ? (size_t)g.M * g.maxC : 0);
    s.dm = cv.take<float>((size_t)g.G * d->C[d->L - 1]);
    s.cst = cv.take<float>((size_t)5 * g.maxC);
    size_t dwmax = 0;
    for (int l = 0; l < d->L; ++l) {
        int nsplit, kp_pad;
        dw_plan(g.M, d->C[l], g.Cin[l], &nsplit, &kp_pad);
        size_t need = (size_t)nsplit * d->C[l] * kp_pad;
        // the fused dA+dW kernels (large M only) write one C_l x C_{l-1} partial per worker, at most kMaxStatBlocks of them
        const size_t fused = (l > 0 && g.M >= 8192) ? (size_t)kMaxStatBlocks * d->C[l] * d->C[l - 1] : 0;
        need = fused > need ? fused : need;
        dwmax = need > dwmax ? need : dwmax;
    }
    if (L.delayed) {  // the per-source-point dW_f partials
        int nsplit, kp_pad;
        dw_plan(d->B * d->N, d->C[0], d->D, &nsplit, &kp_pad);
        const size_t a = (size_t)nsplit * d->C[0] * kp_pad;
        dwmax = a > dwmax ? a : dwmax;
    }
    s.dwslab = cv.take<float>(dwmax);
    s.src = cv.take<float>(L.delayed ? (size_t)d->B * d->N * d->C[0] : 0);
    s.xslab = cv.take<float>(L.delayed ? (size_t)scatter_dz_splits(d->B * d->N) * d->C[0] * 4 : 0);
    s.mom = cv.take<double>((!d->group_all && d->D == 0) ? xyz0_moment_doubles() : 0);
    s.bytes = cv.bytes();
    return s;
}

// the call's workspaces and tensors; the statistics every layer keeps live in `saved`
static void sa_level_bind(SaLevel *L, void *saved, void *scratch, const float *xyz, const float *points, const float *const *conv_w,
                          const float *const *gamma, hipStream_t st) {
    L->sv = sa_saved_layout(*L, saved);
    L->sc = sa_scratch_layout(*L, scratch);
    L->xyz = xyz, L->points = points, L->conv_w = conv_w, L->st = st;
    for (int l = 0; l < L->d->L; ++l) {
        BnLayer &b = L->bn[l];
        b.C = L->d->C[l], b.gamma = gamma[l];
        b.mean = L->sv.mean[l], b.istd = L->sv.istd[l], b.scale = L->sv.scale[l], b.shift = L->sv.shift[l];
    }
}

// A/B switches (PNPP_NO_POOL_FUSION=1: pooling stays a pass of its own over Z; PNPP_NO_POOL_BWD_FUSION=1: so does its backward)
static bool pool_fused_on() { static const bool on = env_int("PNPP_NO_POOL_FUSION", 0) == 0; return on; }
static bool pool_bwd_fused_on() { static const bool on = env_int("PNPP_NO_POOL_BWD_FUSION", 0) == 0; return on; }

// ---- forward ----
static int sa_level_fwd(const pnpp_sa_desc *d, const pnpp_sa_fwd_args *a, hipStream_t st, SaLevel *L) {
    PNPP_TRY(sa_level_plan(d, L));
    PNPP_REQUIRE(a && a->xyz && a->new_xyz && a->out && a->saved && a->scratch, PNPP_ERR_ARG, "sa_forward: null pointer");
    PNPP_REQUIRE(d->D == 0 || a->points, PNPP_ERR_ARG, "sa_forward: D=%d but points is null", d->D);
    PNPP_REQUIRE(d->group_all || a->centre_idx, PNPP_ERR_ARG, "sa_forward: centre_idx is null");
    for (int l = 0; l < d->L; ++l) {
        PNPP_REQUIRE(a->conv_w[l] && a->conv_b[l] && a->bn_w[l] && a->bn_b[l] && a->bn_rm[l] && a->bn_rv[l], PNPP_ERR_ARG,
                     "sa_forward: null parameter pointer in layer %d", l);
        BnLayer &b = L->bn[l];
        b.bias = a->conv_b[l], b.beta = a->bn_b[l], b.rm = a->bn_rm[l], b.rv = a->bn_rv[l];
        b.nbt = d->training ? (long long *)a->bn_nbt[l] : nullptr;
    }
    sa_level_bind(L, a->saved, a->scratch, a->xyz, a->points, a->conv_w, a->bn_w, st);
    L->hyper = BnHyper{d->momentum, d->eps, d->training ? 1 : 0};
    return PNPP_OK;
}

// 1. centres and neighbours (pointnet_pp_8dir.py:23-31)
static int sa_fwd_group(const SaLevel &L, const pnpp_sa_fwd_args *a) {
    const pnpp_sa_desc *d = L.d;
    const SaSaved &sv = L.sv;
    if (d->group_all) return PNPP_OK;   // the centres are the origin: written by the pooling launch that ends this forward
    PNPP_REQUIRE(d->S <= d->N, PNPP_ERR_RANGE, "sa_forward: npoint=%d > N=%d", d->S, d->N);
    if (a->neighbour_idx == sv.idx) return PNPP_OK;   // grouped ahead of time by pnpp_sa_group_pair: everything is already in place
    if (!a->neighbour_idx)   // the neighbour search gathers its own queries and writes the centre coordinates on the way
        return launch_knn_centres(a->xyz, a->centre_idx, d->B, d->S, d->N, d->K, sv.idx, a->new_xyz, sv.new_xyz, L.st);
    PNPP_TRY(launch_gather_centres(a->xyz, a->centre_idx, d->B, d->N, d->S, a->new_xyz, sv.new_xyz, L.st));
    hipError_t e = hipMemcpyAsync(sv.idx, a->neighbour_idx, (size_t)L.g.M * sizeof(int32_t), hipMemcpyDeviceToDevice, L.st);
    PNPP_REQUIRE(e == hipSuccess, PNPP_ERR_LAUNCH, "sa_forward: neighbour copy failed: %s", hipGetErrorString(e));
    return PNPP_OK;
}

// Layer l's BatchNorm: training from the nslab partial sums in sc.slab (exchanged over the ranks first under SyncBN), eval from the
// running statistics.  tail: what else rides in the launch (the pooled output, a group_all level's centres).
static int sa_fwd_finalize(const SaLevel &L, int l, int nslab, const PoolTail *tail = nullptr) {
    StatsView V;
    if (L.d->training) PNPP_TRY(stats_exchange(L.sc.slab, nslab, L.d->C[l], L.count(), L.st, &V));
    return launch_bn_finalize_fwd(V, L.count(), L.bn[l], L.hyper, L.st, tail);
}

// layer l's product; layer 1 of a level on raw coordinates is the product that also finishes layer 0's BatchNorm from (mom, nmom)
static int sa_fwd_gemm(const SaLevel &L, int l, const AOperand &A, const BOperand &W, const Epilogue &E, const double *mom, int nmom, int *ns) {
    if (L.xyz0 && l == 1)
        return launch_wsf0(L.layer0_operand(), L.g.M, L.weight(0, 0), mom, nmom, L.bn[0], L.hyper, L.weight(1, 0), E, ns, L.st);
    return launch_gemm(A, W, L.g.M, L.d->C[l], L.g.Kd[l], E, ns, L.st);
}

// delayed layer 0: P = F W_f^T on the source points, then Z = P[idx] + W_xyz (x - c) with statistics
static int sa_fwd_delayed0(const SaLevel &L, const AOperand &geo) {
    const pnpp_sa_desc *d = L.d;
    AOperand F;
    F.a = L.points, F.lda = d->D;
    BOperand Wf = L.w0_features();
    Wf.trans = 1, Wf.rows = d->D;
    int nslab = 0;
    PNPP_TRY(launch_gemm(F, Wf, d->B * d->N, d->C[0], d->D, store_to(L.sc.src, d->C[0]), nullptr, L.st));
    PNPP_TRY(launch_gather_rel_stats(L.sc.src, geo, L.conv_w[0], L.g.Cin[0], L.g.M, d->C[0], L.sv.z[0], d->training ? L.sc.slab : nullptr,
                                     &nslab, L.st));
    return sa_fwd_finalize(L, 0, nslab);
}

static int sa_forward_impl(const pnpp_sa_desc *d, const pnpp_sa_fwd_args *a, hipStream_t st) {
    SaLevel L;
    PNPP_TRY(sa_level_fwd(d, a, st, &L));
    const SaGeom &g = L.g;
    const SaSaved &sv = L.sv;
    const SaScratch &sc = L.sc;
    PNPP_TRY(sa_fwd_group(L, a));
    // 2. conv -> BN -> ReLU chain; BN apply + ReLU of layer l-1 happen inside layer l's operand loader
    const int Lm = d->L - 1;
    bool pooled = false;
    int nmom = 0;
    const double *mom = sc.mom;   // a level on raw coordinates, training: the moment partials layer 0's statistics come from
    for (int l = 0; l < d->L; ++l) {
        if (L.xyz0 && l == 0) {   // no product: layer 1's launch builds this layer from the coordinates
            if (!d->training) PNPP_TRY(sa_fwd_finalize(L, 0, 0));
            else if (a->neighbour_idx == sv.idx && L.pair_moments) mom = sv.mom, nmom = knn_pair_moment_partials(d->B, d->S, d->N);
            else PNPP_TRY(launch_rel_moments(L.layer0_operand(), g.M, sc.mom, &nmom, st));
            continue;
        }
        const AOperand A = L.input_of(l);
        if (l == 0 && L.delayed) {
            PNPP_TRY(sa_fwd_delayed0(L, A));
            continue;
        }
        Epilogue E = store_to(sv.z[l], d->C[l]);
        BOperand W = L.weight(l, g.Cin[l]);  // the conv weight is read in place; layer 0 maps features-first k' to xyz-first columns
        W.trans = 1, W.perm_D = l == 0 ? d->D : -1;
        if (!d->training) {
            PNPP_TRY(sa_fwd_finalize(L, l, 0));
            PNPP_TRY(sa_fwd_gemm(L, l, A, W, E, mom, nmom, nullptr));
            continue;
        }
        E.mode = E_STORE_STATS, E.slab = sc.slab;
        // last layer of a level with 32-row neighbourhoods: the max over the neighbourhood is taken from the GEMM's accumulators
        // and finished by the statistics launch (sv.zmax holds the extreme pre-BN values; the backward pass reads them too)
        const bool pool_here = l == Lm && l > 0 && pool_fused_on() && gemm_pools_in_epilogue(A, g.M, d->C[l], g.Kd[l], d->K);
        PoolTail T;
        T.G = g.G;
        if (pool_here) {
            E.pool_ext = sv.zmax, E.pool_arg = sv.arg, E.pool_gamma = L.bn[l].gamma;
            T.pool_ext = sv.zmax, T.pool_out = a->out, T.pool_arg = sv.arg;
        }
        if (d->group_all) T.origin_a = a->new_xyz, T.origin_b = sv.new_xyz, T.norigin = g.G * 3;
        int nslab = 0;
        PNPP_TRY(sa_fwd_gemm(L, l, A, W, E, mom, nmom, &nslab));
        PNPP_TRY(sa_fwd_finalize(L, l, nslab, &T));
        pooled = pool_here;
    }
    // 3. max over the neighbourhood (pointnet_pp_8dir.py:42-43), unless the last layer's launches have taken it
    // (the split form's partials go to dy[0], M x C floats idle in the forward pass: >= the K/64 partials per (group, channel))
    if (!pooled) PNPP_TRY(launch_pool_fwd(sv.z[Lm], sv.scale[Lm], sv.shift[Lm], g.G, d->K, d->C[Lm], a->out, sv.arg, st,
                             d->group_all ? a->new_xyz : nullptr, d->group_all ? sv.new_xyz : nullptr, d->group_all ? g.G * 3 : 0,
                             sc.dy[0], L.keeps_zmax ? sv.zmax : nullptr));
    return PNPP_OK;
}

// ---- backward: sa_backward_impl drives the steps below, top layer first ----
static int sa_level_bwd(const pnpp_sa_desc *d, const pnpp_sa_bwd_args *a, hipStream_t st, SaLevel *L) {
    PNPP_TRY(sa_level_plan(d, L));
    PNPP_REQUIRE(a && a->xyz && a->dout && a->saved && a->scratch, PNPP_ERR_ARG, "sa_backward: null pointer");
    for (int l = 0; l < d->L; ++l)
        PNPP_REQUIRE(a->conv_w[l] && a->bn_w[l] && a->d_conv_w[l] && a->d_conv_b[l] && a->d_bn_w[l] && a->d_bn_b[l], PNPP_ERR_ARG,
                     "sa_backward: null pointer in layer %d", l);
    L->want_dpoints = d->D > 0 && a->dpoints != nullptr;
    // a grouped level returns dF through the generic GEMM (scalar stores) and the row scatter, which take any width
    // (tests/test_gpu_cls_bands.py: D = 3); the whole-cloud level's paired dA + dW launch stays with the widths it was written for
    if (L->want_dpoints && d->group_all)
        PNPP_REQUIRE(d->D % 4 == 0, PNPP_ERR_ARG, "sa_backward: feature width D=%d must be a multiple of 4", d->D);
    sa_level_bind(L, const_cast<void *>(a->saved), a->scratch, a->xyz, a->points, a->conv_w, a->bn_w, st);
    for (int l = 0; l < d->L; ++l) L->dbn[l] = BnGrads{a->d_bn_w[l], a->d_bn_b[l], a->d_conv_b[l]};
    return PNPP_OK;
}

struct SaBwdState {   // what one step of the backward driver leaves for the next
    int cur = 0;                 // sc.dy[cur] holds dY of the layer being processed; sc.dy[cur ^ 1] is free
    bool dz_ready = false;       // small-M levels: sc.dzbuf already holds dZ of the layer about to be processed
    bool dpoints_done = false;   // layer 0's dW launch has written the feature gradient as well
};

// the view layer l's BatchNorm-backward sums (nslab partials in sc.slab) are finalised from
static int sa_bwd_stats(const SaLevel &L, int l, int nslab, StatsView *V) {
    V->slab = L.sc.slab, V->nslab = nslab;
    if (L.d->training) PNPP_TRY(stats_exchange(L.sc.slab, nslab, L.d->C[l], L.count(), L.st, V));
    return PNPP_OK;
}

// A ridden reduction reads its partial slabs in the launch that writes this level's statistics slabs and dm.  The two levels may
// share one scratch buffer (the layouts differ, and everything else this level writes is ordered behind that launch): true when
// neither region lies over what the tail reads.  The regions are taken up to the next carved one (sa_scratch_layout's order).
static bool tail_clear_of(const SaTail &T, const SaScratch &sc) {
    auto hits = [&](const SlabReduceArgs &R) {
        const char *lo = (const char *)R.slab, *hi = lo + (size_t)R.nsplit * R.Nc * R.kp_pad * sizeof(float);
        auto over = [&](const void *b, const void *e) { return lo < (const char *)e && (const char *)b < hi; };
        return over(sc.slab, sc.dy[0]) || over(sc.dm, sc.cst);
    };
    return !(hits(T.R1) || (T.kind == PNPP_SA_TAIL_SLAB_REDUCE2 && hits(T.R2)));
}

// The top: the pooled gradient through max + ReLU, and the top layer's BatchNorm-backward constants (sc.cst).
// A level with few groups (group_all: one per cloud) whose dZ is materialised anyway: the finalisation launch takes the pooled
// gradient as it is -- no pool_bwd launch, no dm tensor (PNPP_NO_POOL_BWD_FUSION=1 keeps the launch)
static int sa_bwd_top(const SaLevel &L, const pnpp_sa_bwd_args *a, SaBwdState *S) {
    const pnpp_sa_desc *d = L.d;
    const SaGeom &g = L.g;
    const SaSaved &sv = L.sv;
    const SaScratch &sc = L.sc;
    const int Lm = d->L - 1;
    const bool pooled_src = pool_bwd_fused_on() && L.small && g.G <= 64 && L.keeps_zmax && (d->C[Lm] & 3) == 0 &&
                            !(d->training && stats_sync_on());
    AOperand dz_top = L.dz_operand(Lm, 0);
    S->dz_ready = L.small;
    if (pooled_src) {
        if (L.ride) PNPP_TRY(launch_slab_tail(*L.ride, L.st));   // no pooling launch to ride in: the launch it would have been
        dz_top.a = a->dout;   // the dZ job masks it itself
        PooledSource ps;
        ps.dout = a->dout, ps.zsel = sv.zmax, ps.scale = sv.scale[Lm], ps.shift = sv.shift[Lm], ps.G = g.G;
        return launch_bn_finalize_bwd(StatsView(), L.count(), d->training, L.bn[Lm], sc.cst, L.dbn[Lm], L.st, L.dz_side(&dz_top), &ps);
    }
    int nslab = 0;
    const SaTail *ride = L.ride;
    if (ride && !tail_clear_of(*ride, sc)) {   // this level's workspace lies over the slabs the tail reads: the tail goes first
        PNPP_TRY(launch_slab_tail(*ride, L.st));
        ride = nullptr;
    }
    PNPP_TRY(launch_pool_bwd(a->dout, sv.arg, sv.z[Lm], sv.scale[Lm], sv.shift[Lm], sv.mean[Lm], sv.istd[Lm], g.G, d->K, d->C[Lm], sc.dm,
                             sc.slab, &nslab, L.st, L.keeps_zmax ? sv.zmax : nullptr, ride));
    StatsView V;
    PNPP_TRY(sa_bwd_stats(L, Lm, nslab, &V));
    return launch_bn_finalize_bwd(V, L.count(), d->training, L.bn[Lm], sc.cst, L.dbn[Lm], L.st, L.dz_side(&dz_top));
}

// The level's last reduction, which nothing in the backward pass reads: launched here, or handed to the caller (pnpp_sa_backward_ex)
static int sa_bwd_tail(const SaLevel &L, const SaTail &T) {
    if (!L.defer) return launch_slab_tail(T, L.st);
    *L.defer = T;
    return PNPP_OK;
}

// dZ_l as layer l's launches read it: rebuilt on the fly, or -- small-M levels, where every consumer would rebuild it per
// 32 x 32 tile -- written out once (by the finalisation before, or here)
static int sa_bwd_dz(const SaLevel &L, int l, SaBwdState *S, AOperand *dz) {
    *dz = L.dz_operand(l, S->cur);
    if (!L.small) return PNPP_OK;
    if (!S->dz_ready) PNPP_TRY(launch_dz_materialize(*dz, L.g.M, L.d->C[l], L.sc.dzbuf, L.st));
    S->dz_ready = false;
    *dz = AOperand();
    dz->mode = A_PLAIN, dz->a = L.sc.dzbuf, dz->lda = L.d->C[l];
    return PNPP_OK;
}

// Layers 1 and 0 of a level on raw coordinates end the pass in two launches: layer 1's backward rebuilds Z_0 from the coordinates,
// keeps dY_0 on chip and hands layer 0's parameter gradients to the launch that reduces dW_1 (gemm_wsx_kernels.hip)
static int sa_bwd_xyz0_tail(const SaLevel &L, const pnpp_sa_bwd_args *a, const AOperand &dz) {
    const pnpp_sa_desc *d = L.d;
    const SaGeom &g = L.g;
    int workers = 0, rc = PNPP_OK, C = d->C[1];
    const bool taken = try_launch_wsx(dz, L.weight(1, C), g.M, C, d->C[0], L.layer0_operand(), L.conv_w[0], g.Cin[0], L.sv.scale[0],
                                      L.sv.shift[0], L.sc.dwslab, L.sc.slab, &workers, L.st, &rc);
    // the forward pass of this level kept no Z_0: there is no generic path to fall back to
    PNPP_REQUIRE(taken, PNPP_ERR_ARG, "sa_backward: the coordinate-level backward kernel does not take this call (alignment?)");
    PNPP_TRY(rc);
    const SlabReduceArgs R1{L.sc.dwslab, workers, C, 64, 64, -1, a->d_conv_w[1], g.Cin[1]};
    return launch_xyz0_post(R1, L.sc.slab, L.weight(0, 0), L.bn[0], L.count(), d->training, a->d_conv_w[0], g.Cin[0], L.dbn[0], L.st);
}

// Delayed layer 0 ends the pass: G = dZ_0 summed per source point (dW_xyz = dZ_0^T (x - c) in the same pass); dW_f = G^T F, dF = G W_f
static int sa_bwd_delayed0(const SaLevel &L, const pnpp_sa_bwd_args *a, const AOperand &dz) {
    const pnpp_sa_desc *d = L.d;
    const SaScratch &sc = L.sc;
    const int C = d->C[0], R = d->B * d->N, ldw = L.g.Cin[0];
    PNPP_TRY(launch_scatter_dz(dz, L.layer0_operand(), d->B, d->S * d->K, C, sc.src, sc.xslab, L.st));
    AOperand G, F;
    G.a = sc.src, G.lda = C;
    F.a = L.points, F.lda = d->D;
    int nsplit, kp_pad;
    dw_plan(R, C, d->D, &nsplit, &kp_pad);
    const BOperand Wf = L.w0_features();
    const Epilogue E = store_to(a->dpoints, d->D);
    bool paired = false;
    if (L.want_dpoints) {  // dW_f = G^T F and dF = G W_f only share G: one launch
        int rc = PNPP_OK;
        paired = try_launch_da_dw(G, Wf, R, d->D, C, E, nullptr, F, d->D, sc.dwslab, &nsplit, &kp_pad, L.st, &rc);
        if (paired) PNPP_TRY(rc);
    }
    if (!paired) PNPP_TRY(launch_dw(G, C, F, d->D, R, sc.dwslab, nsplit, kp_pad, L.st));
    // both partial sets of W_0 -- coordinate columns 0..2, feature columns 3.. -- in one launch
    SaTail T;
    T.kind = PNPP_SA_TAIL_SLAB_REDUCE2;
    T.R1 = SlabReduceArgs{sc.xslab, scatter_dz_splits(R), C, 4, 3, -1, a->d_conv_w[0], ldw};
    T.R2 = SlabReduceArgs{sc.dwslab, nsplit, C, kp_pad, d->D, -1, a->d_conv_w[0] + 3, ldw};
    PNPP_TRY(sa_bwd_tail(L, T));
    if (L.want_dpoints && !paired) PNPP_TRY(launch_gemm(G, Wf, R, d->D, C, E, nullptr, L.st));
    return PNPP_OK;
}

// One layer: dY_{l-1} (l > 0), dW_l, then the launch that reduces dW_l's partials and (l > 0) finalises layer l-1's sums into sc.cst.
static int sa_bwd_layer(const SaLevel &L, const pnpp_sa_bwd_args *a, int l, const AOperand &dz, SaBwdState *S) {
    const pnpp_sa_desc *d = L.d;
    const SaGeom &g = L.g;
    const SaSaved &sv = L.sv;
    const SaScratch &sc = L.sc;
    const int C = d->C[l];
    const AOperand a2 = L.input_of(l);
    int nsplit, kp_pad;
    dw_plan(g.M, C, g.Cin[l], &nsplit, &kp_pad);
    int fused_slabs = 0, nslab_next = 0;
    bool pair_done = false;
    if (l > 0) {
        // dY_{l-1} = (dZ_l * W_l) masked by ReLU'(layer l-1), with layer l-1's BN-backward sums; where the
        // weights-stationary kernel applies, dW_l = dZ_l^T * relu(bn(Z_{l-1})) is accumulated in the same launch
        Epilogue E;
        E.mode = E_MASK_STATS;
        E.c = sc.dy[S->cur ^ 1], E.ldc = d->C[l - 1], E.slab = sc.slab, E.zp = sv.z[l - 1];
        E.scale = sv.scale[l - 1], E.shift = sv.shift[l - 1], E.mu = sv.mean[l - 1], E.istd = sv.istd[l - 1];
        E.dwslab = sc.dwslab, E.dw_ld = d->C[l - 1];
        const BOperand W = L.weight(l, C);
        int rc = PNPP_OK;
        pair_done = try_launch_da_dw(dz, W, g.M, d->C[l - 1], C, E, &nslab_next, a2, g.Cin[l], sc.dwslab, &nsplit, &kp_pad, L.st, &rc,
                                     a->d_conv_w[l], g.Cin[l]);   // small-M level: dA and dW of this layer go out as one launch
        if (pair_done) PNPP_TRY(rc);
        else PNPP_TRY(launch_gemm(dz, W, g.M, d->C[l - 1], C, E, &nslab_next, L.st, &fused_slabs));
    }
    const bool xyz_only = l == 0 && d->D == 0 && (a2.mode == A_GATHER || (a2.mode == A_CONCAT && g.M >= 8192)) &&
                          dw_xyz_splits(g.M) <= nsplit * (kp_pad / 4);
    if (xyz_only) {  // C x 3 gradient: streaming kernel (the MFMA tiles would be 95 % padding)
        PNPP_TRY(launch_dw_xyz(dz, C, a2, g.M, sc.dwslab, L.st));
        nsplit = dw_xyz_splits(g.M), kp_pad = 4;
    } else if (fused_slabs == 0 && !pair_done) {  // dW_l = dZ_l^T * A_l as its own launch (layer 0, group_all layers, odd shapes)
        // group_all layer 0 with a feature gradient to return: dW_0 and dF = dZ_0 W_f only share dZ_0 -- one launch
        if (l == 0 && L.want_dpoints && d->group_all) {
            int rc = PNPP_OK;
            S->dpoints_done = try_launch_da_dw(dz, L.w0_features(), g.M, d->D, C, store_to(a->dpoints, d->D), nullptr, a2, g.Cin[0],
                                               sc.dwslab, &nsplit, &kp_pad, L.st, &rc);
            if (S->dpoints_done) PNPP_TRY(rc);
        }
        if (!S->dpoints_done) PNPP_TRY(launch_dw(dz, C, a2, g.Cin[l], g.M, sc.dwslab, nsplit, kp_pad, L.st));
    }
    if (l == 0) {
        SaTail T;
        T.kind = PNPP_SA_TAIL_SLAB_REDUCE;
        T.R1 = SlabReduceArgs{sc.dwslab, nsplit, C, kp_pad, g.Cin[l], d->D, a->d_conv_w[l], g.Cin[l]};
        return sa_bwd_tail(L, T);
    }
    // reduce dW_l's partials and finalise layer l-1's BatchNorm-backward sums in one launch
    const AOperand dz_next = L.dz_operand(l - 1, S->cur ^ 1);  // dY_{l-1} was just written to sc.dy[cur ^ 1]
    StatsView V;
    PNPP_TRY(sa_bwd_stats(L, l - 1, nslab_next, &V));
    const SlabReduceArgs R{sc.dwslab, fused_slabs > 0 ? fused_slabs : nsplit, C, fused_slabs > 0 ? d->C[l - 1] : kp_pad, g.Cin[l], -1,
                           a->d_conv_w[l], g.Cin[l]};
    PNPP_TRY(launch_post_gemm(V, L.count(), d->training, L.bn[l - 1], sc.cst, L.dbn[l - 1], R, L.st, L.dz_side(&dz_next)));
    S->dz_ready = L.small;
    S->cur ^= 1;
    return PNPP_OK;
}

// The feature gradient dF = dZ_0 W_f, unless layer 0's dW launch has written it: a group_all level's rows are the points
// themselves; a grouped level's rows are summed per source point
static int sa_bwd_dpoints(const SaLevel &L, const pnpp_sa_bwd_args *a, const AOperand &dz, const SaBwdState &S) {
    const pnpp_sa_desc *d = L.d;
    const int C = d->C[0];
    if (d->group_all) {
        if (S.dpoints_done) return PNPP_OK;
        return launch_gemm(dz, L.w0_features(), L.g.M, d->D, C, store_to(a->dpoints, d->D), nullptr, L.st);
    }
    float *rows = L.sc.dy[S.cur ^ 1];
    PNPP_TRY(launch_gemm(dz, L.w0_features(), L.g.M, d->D, C, store_to(rows, d->D), nullptr, L.st));
    PNPP_TRY(launch_fill_zero(a->dpoints, (size_t)d->B * d->N * d->D * sizeof(float), L.st));
    return launch_scatter_rows_bwd(rows, L.sv.idx, d->B, d->N, d->D, d->S * d->K, a->dpoints, L.st);
}

static int sa_backward_impl(const pnpp_sa_desc *d, const pnpp_sa_bwd_args *a, hipStream_t st, const SaTail *ride = nullptr,
                            SaTail *defer = nullptr) {
    SaLevel L;
    PNPP_TRY(sa_level_bwd(d, a, st, &L));
    L.ride = ride && ride->kind != PNPP_SA_TAIL_NONE ? ride : nullptr;
    L.defer = defer;
    SaBwdState S;
    PNPP_TRY(sa_bwd_top(L, a, &S));
    for (int l = d->L - 1; l >= 0; --l) {
        AOperand dz;
        PNPP_TRY(sa_bwd_dz(L, l, &S, &dz));
        if (l == 1 && L.xyz0) return sa_bwd_xyz0_tail(L, a, dz);
        if (l == 0 && L.delayed) return sa_bwd_delayed0(L, a, dz);
        PNPP_TRY(sa_bwd_layer(L, a, l, dz, &S));
        if (l == 0 && L.want_dpoints) PNPP_TRY(sa_bwd_dpoints(L, a, dz, S));
    }
    return PNPP_OK;
}

}  // namespace pnpp

using namespace pnpp;

extern "C" size_t pnpp_sa_saved_bytes(const pnpp_sa_desc *d) {
    SaLevel L;
    return sa_level_plan(d, &L) == PNPP_OK ? sa_saved_layout(L, nullptr).bytes : 0;
}
extern "C" size_t pnpp_sa_scratch_bytes(const pnpp_sa_desc *d) {
    SaLevel L;
    return sa_level_plan(d, &L) == PNPP_OK ? sa_scratch_layout(L, nullptr).bytes : 0;
}
extern "C" const int32_t *pnpp_sa_saved_neighbours(const pnpp_sa_desc *d, const void *saved) {
    SaLevel L;
    return sa_level_plan(d, &L) == PNPP_OK && !d->group_all ? sa_saved_layout(L, const_cast<void *>(saved)).idx : nullptr;
}
extern "C" const int32_t *pnpp_sa_saved_argmax(const pnpp_sa_desc *d, const void *saved) {
    SaLevel L;
    return sa_level_plan(d, &L) == PNPP_OK ? sa_saved_layout(L, const_cast<void *>(saved)).arg : nullptr;
}
extern "C" int pnpp_sa_saved_relu_mask(const pnpp_sa_desc *d, const void *saved, const float *xyz, const float *conv_w0, int layer,
                                       uint8_t *out, void *stream) {
    SaLevel L;
    PNPP_TRY(sa_level_plan(d, &L));
    PNPP_REQUIRE(saved && out && layer >= 0 && layer < d->L, PNPP_ERR_ARG, "sa_saved_relu_mask: null pointer or layer %d out of range", layer);
    L.sv = sa_saved_layout(L, const_cast<void *>(saved));
    L.xyz = xyz;
    const SaSaved &sv = L.sv;
    if (layer == 0 && L.xyz0) {   // never stored: rebuilt as the kernels rebuild it
        PNPP_REQUIRE(xyz && conv_w0, PNPP_ERR_ARG, "sa_saved_relu_mask: layer 0 of a level on raw coordinates needs xyz and conv_w0");
        return launch_xyz0_mask(L.layer0_operand(), L.g.M, conv_w0, L.g.Cin[0], sv.scale[0], sv.shift[0], out, as_stream(stream));
    }
    return launch_relu_mask(sv.z[layer], sv.scale[layer], sv.shift[layer], (size_t)L.g.M * d->C[layer], d->C[layer], out, as_stream(stream));
}
static int sa_group_pair_impl(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *lengths, const int32_t *centre1,
                              const int32_t *centre2, void *saved1, float *new_xyz1, void *saved2, float *new_xyz2, void *stream) {
    SaLevel L1, L2;
    PNPP_TRY(sa_level_plan(d1, &L1));
    PNPP_TRY(sa_level_plan(d2, &L2));
    PNPP_REQUIRE(!d1->group_all && !d2->group_all, PNPP_ERR_ARG, "sa_group_pair: both levels must group neighbourhoods");
    PNPP_REQUIRE(d1->B == d2->B && d2->N == d1->S, PNPP_ERR_ARG, "sa_group_pair: level 2 must take level 1's %d centres (got N=%d)",
                 d1->S, d2->N);
    PNPP_REQUIRE(xyz && centre1 && centre2 && saved1 && saved2 && new_xyz1 && new_xyz2, PNPP_ERR_ARG, "sa_group_pair: null pointer");
    const SaSaved s1 = sa_saved_layout(L1, saved1), s2 = sa_saved_layout(L2, saved2);
    return launch_knn_pair(xyz, d1->B, d1->N, centre1, d1->S, d1->K, s1.idx, new_xyz1, s1.new_xyz, centre2, d2->S, d2->K, s2.idx,
                           new_xyz2, s2.new_xyz, L1.pair_moments ? s1.mom : nullptr, as_stream(stream), lengths);
}
extern "C" int pnpp_sa_group_pair(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *centre1,
                                  const int32_t *centre2, void *saved1, float *new_xyz1, void *saved2, float *new_xyz2, void *stream) {
    return sa_group_pair_impl(d1, d2, xyz, nullptr, centre1, centre2, saved1, new_xyz1, saved2, new_xyz2, stream);
}
// ... of a ragged batch: level 1 searches each cloud's first lengths[b] rows (level 2 searches level 1's centres: uniform)
extern "C" int pnpp_sa_group_pair_ragged(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *lengths,
                                         const int32_t *centre1, const int32_t *centre2, void *saved1, float *new_xyz1, void *saved2,
                                         float *new_xyz2, void *stream) {
    PNPP_REQUIRE(lengths, PNPP_ERR_ARG, "sa_group_pair_ragged: null lengths");
    return sa_group_pair_impl(d1, d2, xyz, lengths, centre1, centre2, saved1, new_xyz1, saved2, new_xyz2, stream);
}

extern "C" int pnpp_sa_forward(const pnpp_sa_desc *d, const pnpp_sa_fwd_args *a, void *stream) { return sa_forward_impl(d, a, as_stream(stream)); }
extern "C" int pnpp_sa_backward(const pnpp_sa_desc *d, const pnpp_sa_bwd_args *a, void *stream) { return sa_backward_impl(d, a, as_stream(stream)); }

// ---- a level's trailing reduction handed on (pnpp_sa_tail; the contract is in the header) ----
static SlabReduceArgs tail_args(const pnpp_slab_reduce &r) { return SlabReduceArgs{r.slab, r.nsplit, r.Nc, r.kp_pad, r.Kvalid, r.perm_D, r.out, r.ldo}; }
static pnpp_slab_reduce tail_args(const SlabReduceArgs &R) { return pnpp_slab_reduce{R.slab, R.nsplit, R.Nc, R.kp_pad, R.Kvalid, R.perm_D, R.out, R.ldo}; }
static int tail_in(const pnpp_sa_tail *t, SaTail *T) {
    *T = SaTail();
    if (!t || t->kind == PNPP_SA_TAIL_NONE) return PNPP_OK;
    PNPP_REQUIRE(t->kind == PNPP_SA_TAIL_SLAB_REDUCE || t->kind == PNPP_SA_TAIL_SLAB_REDUCE2, PNPP_ERR_ARG, "sa tail: unknown kind %d", t->kind);
    const int n = t->kind == PNPP_SA_TAIL_SLAB_REDUCE2 ? 2 : 1;
    for (int i = 0; i < n; ++i)
        PNPP_REQUIRE(t->r[i].slab && t->r[i].out && t->r[i].nsplit > 0 && t->r[i].Nc > 0 && t->r[i].Kvalid > 0 && t->r[i].kp_pad >= t->r[i].Kvalid &&
                         t->r[i].ldo > 0, PNPP_ERR_ARG, "sa tail: reduction %d is not one a backward call wrote", i);
    T->kind = t->kind, T->R1 = tail_args(t->r[0]);
    if (n == 2) T->R2 = tail_args(t->r[1]);
    PNPP_REQUIRE(slab_tail_blocks(*T) == t->blocks, PNPP_ERR_ARG, "sa tail: %d blocks, the reduction takes %d", t->blocks, slab_tail_blocks(*T));
    return PNPP_OK;
}
extern "C" int pnpp_sa_backward_ex(const pnpp_sa_desc *d, const pnpp_sa_bwd_args *a, const pnpp_sa_tail *ride, pnpp_sa_tail *defer, void *stream) {
    SaTail in, out;
    PNPP_TRY(tail_in(ride, &in));
    if (defer) memset(defer, 0, sizeof(*defer));
    PNPP_TRY(sa_backward_impl(d, a, as_stream(stream), &in, defer ? &out : nullptr));
    if (defer && out.kind != PNPP_SA_TAIL_NONE) {
        defer->kind = out.kind, defer->blocks = slab_tail_blocks(out);
        defer->r[0] = tail_args(out.R1);
        if (out.kind == PNPP_SA_TAIL_SLAB_REDUCE2) defer->r[1] = tail_args(out.R2);
    }
    return PNPP_OK;
}
extern "C" int pnpp_sa_run_tail(const pnpp_sa_tail *t, void *stream) {
    SaTail T;
    PNPP_TRY(tail_in(t, &T));
    return launch_slab_tail(T, as_stream(stream));
}
