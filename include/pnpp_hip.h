/*
 * pnpp_hip.h -- C ABI of libpnpp_hip.so: the MI355X (gfx950) implementation of the
 * PointNet++ set-abstraction + von-Mises-KL training path of
 * 0xPabloxx/3d-pointcloud-orientation-estimation.
 *
 * The reference has no FFI of its own: its boundary is the Python surface listed in
 * SURVEY.md 8(b).  Each entry point below names the reference interface (file:line under
 * /root/reference) whose work it performs; the Python host in
 * 3d-pointcloud-orientation-estimation_amd/ keeps the reference's names on top of these.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - Every pointer is a DEVICE pointer unless the name ends in _host.
 *   - Tensors are dense row-major float32; indices are int32 on the device
 *     (the Python host converts to the reference's int64 at its own boundary).
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises, allocates or frees.  Outputs and workspaces are caller-owned.
 *   - Return value: PNPP_OK or a negative pnpp_status; pnpp_last_error() gives the text.
 *     No exception crosses the ABI.  Functions are re-entrant; the only global state is
 *     the thread-local last-error string, an immutable device-property cache and the two
 *     process-wide switches (matmul precision, BatchNorm statistics exchange).
 */
#ifndef PNPP_HIP_H
#define PNPP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PNPP_OK = 0,
    PNPP_ERR_ARG = -1,      /* bad shape / null pointer / unsupported size: Python raises ValueError   */
    PNPP_ERR_RANGE = -2,    /* k > N and similar: Python raises RuntimeError like torch.topk           */
    PNPP_ERR_LAUNCH = -3,   /* hipLaunch / hipGetLastError failure: Python raises RuntimeError         */
    PNPP_ERR_WORKSPACE = -4 /* workspace too small                                                       */
} pnpp_status;

const char *pnpp_last_error(void);
int pnpp_abi_version(void);

/* Opt-in per-launch timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 * pnpp_profile_enable(1) starts recording one event pair around every kernel the library launches (not
 * thread-safe, adds ~2 us per launch: never on while throughput is being timed); pnpp_profile_report
 * synchronises the recorded events and writes one line per distinct launch tag,
 * "<kernel and shape tag>\t<launches>\t<total ms>\n", into buf (truncated to buflen), then clears.
 * Returns the number of distinct tags, or a negative pnpp_status. */
int pnpp_profile_enable(int on);
int pnpp_profile_report(char *buf_host, size_t buflen);

/* ------------------------------------------------------------------------------------------
 * Index primitives
 * ---------------------------------------------------------------------------------------- */

/* models/base.py:20-27  square_distance(src (B,S,3), dst (B,N,3)) -> out (B,S,N).
 * Bit-equal to the ATen CPU evaluation order (fmaf-chained dot, unfused norms). */
int pnpp_square_distance(const float *src, const float *dst, int B, int S, int N, float *out, void *stream);

/* models/base.py:29-35  query_ball_point(new_xyz, xyz, nsample) == kNN.
 * new_xyz (B,S,3), xyz (B,N,3) -> idx (B,S,k) int32, ascending (distance, index).
 * The k smallest by the bit-exact float32 recipe; lowest index wins ties. */
int pnpp_knn(const float *new_xyz, const float *xyz, int B, int S, int N, int k, int32_t *idx, void *stream);

/* PointNet++Demo.py:8-29  farthest_point_sample with the start indices injected.
 * xyz (B,N,3), start (B) -> out (B,npoint) int32. */
int pnpp_fps(const float *xyz, int B, int N, int npoint, const int32_t *start, int32_t *out, void *stream);

/* PointNet++Demo.py:49-70  query_ball_point(radius, nsample, xyz, new_xyz) -> idx (B,S,nsample) int32.
 * A point is a member when !(d > r2), d the float32 squared distance and r2 a float32 threshold.
 *   pnpp_ball_query      r2 = (float)((double)radius * (double)radius): the radius is a float32 BEFORE it is squared.  For a radius that
 *                        float32 does not hold exactly (0.2, 0.4, ...) this can sit one float32 away from what the reference compares
 *                        against, float32(radius ** 2) of the python float (Demo.py:65): above for 0.05, 0.1, 0.2, 0.4, 0.8, below
 *                        for 0.35, 0.45.  Kept for callers whose radius is a float32 to begin with.
 *   pnpp_ball_query_r2   takes the threshold itself; hand it float32(radius ** 2), rounded once from double, for the reference's rule
 *                        (what pnpp_hip.ops.ball_query does). */
int pnpp_ball_query(const float *new_xyz, const float *xyz, int B, int S, int N, float radius, int nsample,
                    int32_t *idx, void *stream);
int pnpp_ball_query_r2(const float *new_xyz, const float *xyz, int B, int S, int N, float r2, int nsample, int32_t *idx,
                       void *stream);

/* models/pointnet_pp_8dir.py:28  per-cloud uniform random subset of size npoint out of N, without
 * replacement, in random order -- the device-side replacement of B host `torch.randperm(N)[:npoint]`
 * calls (throughput mode; parity mode replays the CPU generator on the host and passes the indices in).
 * Counter-based: the result is a pure function of (seed, stream_id, b).  out (B,npoint) int32. */
int pnpp_sample_random(uint64_t seed, uint64_t stream_id, int B, int N, int npoint, int32_t *out, void *stream);
/* dataloader_single_peak_vonMises.py:12-14 (and the two other dataloaders): sample_pts = np.random.choice(len, num,
 * replace=len<num) rows of a cloud -- on the device, for a bank of full clouds resident in HBM: bank (n_clouds,Lmax,3),
 * lengths (n_clouds) valid rows per cloud, cloud_ids (B) bank row of every batch slot (NULL: slot b reads cloud b).
 * out (B,num,3): an ordered uniform subset without replacement where lengths >= num, uniform draws with replacement
 * where 0 < lengths < num, zeros for an empty cloud.  Pure function of (seed, stream_id, slot); any Lmax (the LDS key table is sized by num, not by the cloud). */
int pnpp_subsample_points(uint64_t seed, uint64_t stream_id, const float *bank, const int32_t *lengths,
                          const int32_t *cloud_ids, int B, int Lmax, int num, float *out, void *stream);
/* Same, with the stream id read from DEVICE memory at kernel time: stream_id = stream_id_dev[0] + offset, and the
 * kernel post-increments stream_id_dev[0] once every workgroup has read it -- the launch can be captured into a
 * hipGraph and still draws fresh centres on every replay.  stream_id_dev points at TWO uint64 words: the counter and
 * a ticket word that must be zero before the first call (the kernel leaves it zero). */
int pnpp_sample_random_dev(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N, int npoint,
                           int32_t *out, void *stream);
/* Two consecutive pnpp_sample_random_dev draws (the centres of two stacked set-abstraction levels: pointnet_pp_8dir.py:28
 * of sa1 and sa2) in one launch: out1 (B,npoint1) uses the counter's value, out2 (B,npoint2) the next one, the counter
 * advances by two -- bit-identical to the two separate calls. */
int pnpp_sample_random_dev2(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N1, int npoint1, int32_t *out1,
                            int N2, int npoint2, int32_t *out2, void *stream);

/* Ragged batches of the index primitives: xyz stays the padded (B,N,3) tensor, lengths (B) int32 in DEVICE memory says how many of
 * cloud b's rows are points.  Each call is its namesake with `lengths` after N; a kernel reads Nv = min(max(lengths[b], 1), N) once per
 * workgroup and uses it wherever the cloud's extent matters, so row b of a result is what the namesake returns for xyz[b, :Nv] alone
 * and no index >= Nv is ever written; the padding rows may hold anything.  Argument checks are the namesake's (against the padded
 * N: the host does not see the lengths) and a NULL lengths is PNPP_ERR_ARG.  What the device cannot refuse:
 *   knn            k > Nv: the list's slots >= Nv repeat slot 0;
 *   fps            npoint > Nv is legal as in the namesake (once every distance is 0 the first maximum is point 0); start[b] < Nv;
 *   ball_query     a centre without a member in its cloud is filled with Nv (cannot occur when the centres are points of the cloud);
 *   sample_random  npoint > Nv: rank r >= Nv repeats rank r mod Nv.  The draw of cloud b is the namesake's at N = Nv for the same
 *                  batch position, bit for bit.  _dev2: lengths belong to the first draw (the second ranks level 1's centres). */
int pnpp_knn_ragged(const float *new_xyz, const float *xyz, int B, int S, int N, const int32_t *lengths, int k, int32_t *idx, void *stream);
int pnpp_fps_ragged(const float *xyz, int B, int N, const int32_t *lengths, int npoint, const int32_t *start, int32_t *out, void *stream);
int pnpp_ball_query_ragged(const float *new_xyz, const float *xyz, int B, int S, int N, const int32_t *lengths, float radius, int nsample,
                           int32_t *idx, void *stream);
int pnpp_ball_query_r2_ragged(const float *new_xyz, const float *xyz, int B, int S, int N, const int32_t *lengths, float r2, int nsample,
                              int32_t *idx, void *stream);
int pnpp_sample_random_ragged(uint64_t seed, uint64_t stream_id, int B, int N, const int32_t *lengths, int npoint, int32_t *out,
                              void *stream);
int pnpp_sample_random_dev_ragged(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N, const int32_t *lengths,
                                  int npoint, int32_t *out, void *stream);
int pnpp_sample_random_dev2_ragged(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N1, const int32_t *lengths,
                                   int npoint1, int32_t *out1, int N2, int npoint2, int32_t *out2, void *stream);

/* models/base.py:4-18  index_points(points (B,N,C), idx (B,M)) -> out (B,M,C); idx is int32, flattened
 * over its trailing dims.  _bwd accumulates dpoints (B,N,C) += scatter(dout) deterministically
 * (dpoints must be zero-initialised by the caller when it wants a pure gradient). */
int pnpp_index_points(const float *points, const int32_t *idx, int B, int N, int C, int M, float *out, void *stream);
int pnpp_index_points_bwd(const float *dout, const int32_t *idx, int B, int N, int C, int M, float *dpoints,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Set abstraction: grouping + 3 x (1x1 conv -> train/eval BatchNorm2d -> ReLU) + max over nsample
 * models/pointnet_pp_8dir.py:21-43 (PointNetSetAbstraction.forward) and its autograd backward.
 * ---------------------------------------------------------------------------------------- */
#define PNPP_MAX_LAYERS 4

typedef struct {
    int B;             /* clouds                                                                  */
    int N;             /* points per cloud going in                                               */
    int S;             /* centres per cloud (npoint); 1 when group_all                            */
    int K;             /* neighbours per centre (nsample); N when group_all                       */
    int D;             /* feature channels of `points` (0 when points is None)                    */
    int L;             /* number of conv/bn layers (3 in every reference model)                   */
    int C[PNPP_MAX_LAYERS]; /* mlp_channels, each a multiple of 32                                */
    int group_all;     /* pointnet_pp_8dir.py:23-26                                               */
    int training;      /* 1: batch statistics + running-stat update; 0: running statistics        */
    float eps;         /* 1e-5                                                                    */
    float momentum;    /* 0.1                                                                     */
} pnpp_sa_desc;

typedef struct {
    const float *xyz;          /* (B,N,3)                                                          */
    const float *points;       /* (B,N,D) or NULL                                                  */
    const int32_t *centre_idx; /* (B,S) centre indices (unused when group_all)                     */
    const int32_t *neighbour_idx; /* optional (B,S,K): use these neighbours instead of running the kNN
                                  (radius grouping of PointNet++Demo.py:49-70, or injection in tests)  */
    const float *conv_w[PNPP_MAX_LAYERS];   /* (C[l], Cin[l]) = state_dict convs.l.weight, xyz columns first */
    const float *conv_b[PNPP_MAX_LAYERS];   /* (C[l])                                               */
    const float *bn_w[PNPP_MAX_LAYERS];     /* gamma                                                */
    const float *bn_b[PNPP_MAX_LAYERS];     /* beta                                                 */
    float *bn_rm[PNPP_MAX_LAYERS];          /* running_mean (updated in training)                   */
    float *bn_rv[PNPP_MAX_LAYERS];          /* running_var  (updated in training)                   */
    int64_t *bn_nbt[PNPP_MAX_LAYERS];       /* num_batches_tracked (+1 in training) or NULL         */
    float *new_xyz;            /* out (B,S,3)                                                      */
    float *out;                /* out (B,S,C[L-1])                                                 */
    void *saved;               /* activations kept for backward, pnpp_sa_saved_bytes()             */
    void *scratch;             /* transient, pnpp_sa_scratch_bytes()                               */
} pnpp_sa_fwd_args;

typedef struct {
    const float *xyz, *points;
    const float *conv_w[PNPP_MAX_LAYERS];
    const float *bn_w[PNPP_MAX_LAYERS];
    const float *bn_b[PNPP_MAX_LAYERS];
    const float *dout;         /* (B,S,C[L-1]) upstream gradient                                   */
    const void *saved;         /* as written by pnpp_sa_forward                                    */
    void *scratch;             /* pnpp_sa_scratch_bytes()                                          */
    float *d_conv_w[PNPP_MAX_LAYERS];       /* out, same shapes as conv_w                           */
    float *d_conv_b[PNPP_MAX_LAYERS];       /* out (written as exact zeros in training: a bias in front
                                               of a train-mode BatchNorm has zero gradient)         */
    float *d_bn_w[PNPP_MAX_LAYERS], *d_bn_b[PNPP_MAX_LAYERS];
    float *dpoints;            /* out (B,N,D) or NULL                                              */
} pnpp_sa_bwd_args;

size_t pnpp_sa_saved_bytes(const pnpp_sa_desc *d);
size_t pnpp_sa_scratch_bytes(const pnpp_sa_desc *d);
int pnpp_sa_forward(const pnpp_sa_desc *d, const pnpp_sa_fwd_args *a, void *stream);
int pnpp_sa_backward(const pnpp_sa_desc *d, const pnpp_sa_bwd_args *a, void *stream);

/* A level's trailing weight-gradient reduction as a value.  The last reduction of a level's backward pass (layer 0's dW partials
 * summed into d_conv_w[0]) is read by nobody until the optimiser runs, and the level below opens its backward pass with a pooling
 * launch that does not read it either: the two can share one launch.  pnpp_sa_backward_ex can leave that reduction out and describe
 * it here instead; the next level's call takes the description and runs it in extra workgroups behind its pooling launch
 * ("rides"), or pnpp_sa_run_tail launches it on its own.  The arithmetic, the summation order and the stores are those of the
 * launch pnpp_sa_backward makes: results are bit-identical whichever way the tail runs.
 *
 * CONTRACT.  A tail points into the `scratch` of the call that deferred it (the partial slabs) and into that call's d_conv_w[0].
 * Both must stay allocated and UNTOUCHED until the tail has run: whatever else would use that scratch buffer runs the tail first
 * (pnpp_sa_run_tail).  The one exception is the call that takes the tail as `ride`: it may be given the same buffer, because it
 * checks its own layout against the slabs the tail reads and launches the tail on its own, first, where its opening launch would
 * write over them.  Every deferred tail must be run -- ridden or flushed -- before the gradients are read, at the latest when
 * the backward pass ends.  A tail that is never run is a gradient that is never written. */
typedef enum { PNPP_SA_TAIL_NONE = 0, PNPP_SA_TAIL_SLAB_REDUCE = 1, PNPP_SA_TAIL_SLAB_REDUCE2 = 2 } pnpp_sa_tail_kind;
typedef struct {            /* out[c][perm(k)] = sum over s < nsplit of slab[s][c][k], c < Nc, k < Kvalid                  */
    const float *slab;      /* nsplit partials of Nc x kp_pad floats                                                        */
    int nsplit, Nc, kp_pad, Kvalid;
    int perm_D;             /* < 0: k as it is; else features-first -> xyz-first columns (k < perm_D -> k + 3, else k - perm_D) */
    float *out;
    int ldo;
} pnpp_slab_reduce;
typedef struct {
    int kind;               /* pnpp_sa_tail_kind                                                                            */
    int blocks;             /* workgroups (of 256 threads) the reduction takes, as its own launch or as riders             */
    pnpp_slab_reduce r[2];  /* SLAB_REDUCE: r[0]; SLAB_REDUCE2: r[0] (coordinate columns) then r[1] (feature columns)       */
} pnpp_sa_tail;
/* pnpp_sa_backward with the trailing reduction handed on.  ride (may be NULL, may be of kind NONE): a tail deferred by an earlier
 * call; it is run by this call -- behind the opening pooling launch where the level has one and the merged kernel exists for the
 * tail's form, else as an ordinary launch of its own ahead of the level's first.  defer (may be NULL): the level's last reduction
 * is not launched but described in *defer; a level that ends another way (layers 1 and 0 of a level on raw coordinates, a
 * gradient written in place) returns kind NONE and has launched everything.  With both NULL this is pnpp_sa_backward. */
int pnpp_sa_backward_ex(const pnpp_sa_desc *d, const pnpp_sa_bwd_args *a, const pnpp_sa_tail *ride, pnpp_sa_tail *defer, void *stream);
/* launches a deferred tail on its own (the flush): the launch pnpp_sa_backward would have made.  Kind NONE: nothing. */
int pnpp_sa_run_tail(const pnpp_sa_tail *t, void *stream);

/* Grouping of two stacked levels ahead of their forward passes, in ONE launch (models/pointnet_pp_8dir.py:28-31 of sa1 and of
 * sa2: index_points + query_ball_point twice).  Level 2 searches among level 1's centres, which are rows of the same cloud, so
 * once both levels' centre indices are drawn neither search waits for anything: d1 / d2 describe the two levels (d2->N == d1->S),
 * centre1 (B,S1) rows of xyz, centre2 (B,S2) positions among level 1's centres.  Writes the neighbour indices and centre
 * coordinates into saved1 / saved2 (sized by pnpp_sa_saved_bytes) and new_xyz1 (B,S1,3) / new_xyz2 (B,S2,3); pnpp_sa_forward then
 * takes them as already grouped when its neighbour_idx argument IS pnpp_sa_saved_neighbours(d, saved) (and new_xyz is that buffer). */
int pnpp_sa_group_pair(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *centre1,
                       const int32_t *centre2, void *saved1, float *new_xyz1, void *saved2, float *new_xyz2, void *stream);
/* The search of pnpp_sa_group_pair on plain buffers, with the moment partials its level-1 side can sum on the way: idx1 (B,S1,k1),
 * new_xyz1 (B,S1,3), idx2 (B,S2,k2), new_xyz2 (B,S2,3).  mom (optional) receives pnpp_knn_pair_partials(B,S1,N) partials of 16 doubles,
 * the first nine of each being sum rel (x,y,z) and sum rel rel^T (xx,xy,xz,yy,yz,zz) of rel = neighbour - centre over the workgroup's
 * level-1 neighbourhoods (float32 terms, float64 sums, fixed order). */
int pnpp_knn_pair(const float *xyz, int B, int N, const int32_t *centre1, int S1, int k1, int32_t *idx1, float *new_xyz1,
                  const int32_t *centre2, int S2, int k2, int32_t *idx2, float *new_xyz2, double *mom, void *stream);
int pnpp_knn_pair_partials(int B, int S1, int N);
/* The two calls above on a ragged batch (see pnpp_knn_ragged): lengths (B) int32 on the device are level 1's clouds; level 2 searches
 * level 1's centres, which are uniform.  Grid, tile and the number of moment partials are those of the padded N, so a level grouped
 * this way goes through pnpp_sa_forward / pnpp_sa_backward unchanged. */
int pnpp_sa_group_pair_ragged(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *lengths,
                              const int32_t *centre1, const int32_t *centre2, void *saved1, float *new_xyz1, void *saved2,
                              float *new_xyz2, void *stream);
int pnpp_knn_pair_ragged(const float *xyz, int B, int N, const int32_t *lengths, const int32_t *centre1, int S1, int k1, int32_t *idx1,
                         float *new_xyz1, const int32_t *centre2, int S2, int k2, int32_t *idx2, float *new_xyz2, double *mom,
                         void *stream);
/* read-only view of the neighbour indices kept in `saved` ((B,S,K) int32; NULL when group_all) */
const int32_t *pnpp_sa_saved_neighbours(const pnpp_sa_desc *d, const void *saved);
/* read-only view of the max-pool routing kept in `saved`: (B*S, C_last) int32, the position 0..K-1 inside its group of the
 * row that torch.max(x, 3) selected (pointnet_pp_8dir.py:42; first maximum on ties) */
const int32_t *pnpp_sa_saved_argmax(const pnpp_sa_desc *d, const void *saved);
/* diagnostics for parity tests: the ReLU decisions of layer `layer` (0 .. L-1) of this call exactly as its backward pass takes
 * them -- out[M x C_layer] bytes, 1 where F.relu(bn(conv(x))) of pointnet_pp_8dir.py:40-41 lets the gradient pass: the sign of
 * fmaf(Z_l, scale_l, shift_l) on the kept pre-BN activations; layer 0 of a level on raw coordinates keeps no Z_0 and is rebuilt
 * from xyz (B,N,3) and conv_w0 (C_0 x 3) by the same matrix instructions as the kernels (NULL for other levels / layers).
 * A float64 evaluation that is handed these decisions and the max-pool routing above is a smooth function of rounding. */
int pnpp_sa_saved_relu_mask(const pnpp_sa_desc *d, const void *saved, const float *xyz, const float *conv_w0, int layer,
                            uint8_t *out, void *stream);
/* compile-time experiment switches that were on when the library was built (timing experiments that compute WRONG results,
 * in-kernel stamps): 0 in a library that ships -- tests/test_abi.py holds it to 0.  bit 0 PNPP_WS_EXP_NO_MFMA, 1 WSP_EXP,
 * 2 WSX_EXP, 3 WSQ_EXP, 4 WSQ_PLAIN, 5 FCF_EXP, 6 PNPP_STAMPS, 7 WSF_EXP, 8 WD3_PRIO */
unsigned pnpp_build_flags(void);

/* ------------------------------------------------------------------------------------------
 * Fully connected block: y = act(norm(x W^T + b)) with norm in {BatchNorm1d, LayerNorm, none},
 * optional ReLU and inverted dropout by an explicit {0,1} mask.
 * models/pointnet_pp_vonMises.py:32-35, pointnet_pp_8dir.py:81-85, pointnet_pp_mvM.py:82-83.
 * ---------------------------------------------------------------------------------------- */
typedef enum { PNPP_NORM_NONE = 0, PNPP_NORM_BATCH = 1, PNPP_NORM_LAYER = 2 } pnpp_norm;

typedef struct {
    int M, K, N;        /* rows (batch), in features, out features                               */
    int norm;           /* pnpp_norm                                                              */
    int relu;           /* apply ReLU after norm                                                  */
    int training;
    float eps, momentum;
    float drop_scale;   /* 1/(1-p) applied with `mask` / the drawn mask; ignored without dropout   */
} pnpp_fc_desc;

typedef struct {
    const float *x;      /* (M,K)                                                                  */
    const float *w;      /* (N,K)                                                                  */
    const float *b;      /* (N)                                                                    */
    const float *nw, *nb;/* norm affine (N) or NULL                                                */
    float *rm, *rv;      /* BatchNorm running stats or NULL                                        */
    int64_t *nbt;        /* BatchNorm num_batches_tracked (+1 in training) or NULL                 */
    const uint8_t *mask; /* (M,N) dropout keep-mask or NULL                                        */
    uint8_t *mask_out;   /* or: (M,N) keep-mask DRAWN by the kernel (training, BatchNorm, M <= 32):
                            Bernoulli(1 - drop_p) from Philox keyed by rng_seed, stream id rng_counter[0];
                            the kernel post-increments rng_counter[0] (rng_counter[1] is its ticket word,
                            zero on entry and exit); pass it as `mask` to pnpp_fc_backward.  NULL: unused */
    float drop_p;
    uint64_t rng_seed;
    uint64_t *rng_counter;
    float *y;            /* out (M,N)                                                              */
    void *saved;         /* pnpp_fc_saved_bytes()                                                  */
    void *scratch;       /* pnpp_fc_scratch_bytes()                                                */
} pnpp_fc_fwd_args;

typedef struct {
    const float *x, *w, *b, *nw, *nb;
    const uint8_t *mask;
    const float *dy;     /* (M,N)                                                                  */
    const void *saved;
    void *scratch;
    float *dx;           /* (M,K) or NULL                                                          */
    float *dw, *db;      /* (N,K), (N)                                                             */
    float *dnw, *dnb;    /* (N) or NULL                                                            */
} pnpp_fc_bwd_args;

size_t pnpp_fc_saved_bytes(const pnpp_fc_desc *d);
size_t pnpp_fc_scratch_bytes(const pnpp_fc_desc *d);
int pnpp_fc_forward(const pnpp_fc_desc *d, const pnpp_fc_fwd_args *a, void *stream);
int pnpp_fc_backward(const pnpp_fc_desc *d, const pnpp_fc_bwd_args *a, void *stream);
/* y of a BatchNorm block with M > 32 recomputed from its forward call's `saved` (bit-identical to the forward output), so that a
 * caller need not keep y for the backward pass; `mask` as given to the forward call */
int pnpp_fc_recompute_output(const pnpp_fc_desc *d, const void *saved, const uint8_t *mask, float *y, void *stream);

/* ------------------------------------------------------------------------------------------
 * Output heads and losses (forward value and analytic gradient in one launch): csrc/loss_kernels.hip; the one-launch step tails
 * pnpp_vm_fc_head_kl_step(_sample), pnpp_mvm_fc_head_match_step and pnpp_vm_match_loss: csrc/step_tail_kernels.hip; the float64
 * device math they share: csrc/vonmises.h
 * ---------------------------------------------------------------------------------------- */

/* pointnet_pp_vonMises.py:36-37 + train_single_peak_vonMises_KL.py:23-28,83:
 * o (B,2) raw fc3 output -> mu = tanh(o0)*pi, kappa = softplus(o1);
 * loss_vec[b] = KL(vM(mu,kappa) || vM(mu_gt,kappa_gt)) by the reference formula (kappa_p <= 1e-6 branch
 * included, log I0 evaluated as kappa + log(i0e) so kappa >= 89 stays finite where the reference is NaN).
 * d_o (B,2) = d loss_vec[b] / d o[b,:]  (the host scales by the upstream gradient, 1/B for .mean()). */
int pnpp_vm_head_kl(const float *o, const float *mu_gt, const float *kappa_gt, int B, float *mu, float *kappa,
                    float *loss_vec, float *d_o, void *stream);
/* The whole tail of the single-peak step in one launch: o = x W^T + b (the model's fc3: pointnet_pp_vonMises.py:35,
 * W is (2,K)), head activations, KL, .mean() (train_single_peak_vonMises_KL.py:82-84) and their backward:
 * loss_mean[0], dw (2,K), db (2), dx (B,K; may be NULL).  Gradients are written, not accumulated. */
int pnpp_vm_fc_head_kl_step(const float *x, const float *w, const float *b, const float *mu_gt, const float *kappa_gt, int B,
                            int K, float *loss_mean, float *dw, float *db, float *dx, void *stream);
/* The same launch, carrying the NEXT step's centre draw in its idle CUs: workgroup 0 is pnpp_vm_fc_head_kl_step, workgroups 1 .. 2*Bs
 * are pnpp_sample_random_dev2(seed, stream_id_dev, offset, Bs, N1, npoint1, out1, N2, npoint2, out2) -- the draws of
 * models/pointnet_pp_8dir.py:28 for sa1 and sa2 depend on nothing but their counter, so a training loop that keeps (out1, out2)
 * as the centres of its next forward pass draws exactly the sequence it would draw at the start of every step, one launch fewer. */
int pnpp_vm_fc_head_kl_step_sample(const float *x, const float *w, const float *b, const float *mu_gt, const float *kappa_gt, int B,
                                   int K, float *loss_mean, float *dw, float *db, float *dx, uint64_t seed, uint64_t *stream_id_dev,
                                   uint64_t offset, int Bs, int N1, int npoint1, int32_t *out1, int N2, int npoint2, int32_t *out2,
                                   void *stream);
/* The same, followed by the batch mean of train_single_peak_vonMises_KL.py:83 (`loss = kl_von_mises(...).mean()`),
 * in one single-workgroup launch: loss_mean[0] = mean_b loss_vec[b] (fixed-order fp64 sum),
 * d_o_mean (B,2) = d loss_mean / d o.  mu, kappa and loss_vec may be NULL. */
int pnpp_vm_head_kl_mean(const float *o, const float *mu_gt, const float *kappa_gt, int B, float *mu, float *kappa,
                         float *loss_vec, float *loss_mean, float *d_o_mean, void *stream);
/* backward of the activation alone: d_o[b] = (dmu[b]*pi*(1-tanh^2 o0), dkappa[b]*sigmoid(o1)). */
int pnpp_vm_head_bwd(const float *o, const float *dmu, const float *dkappa, int B, float *d_o, void *stream);

/* train_single_peak_vonMises_KL.py:23-28 on its own: values and d/dmu_p, d/dkappa_p. */
int pnpp_vm_kl_single(const float *mu_p, const float *kappa_p, const float *mu_q, const float *kappa_q, int n,
                      float *kl, float *dmu, float *dkappa, void *stream);

/* train_multi_peaks_vonMises_KL.py:38-81 match_loss: per sample K x K cost of the clamped / wrapped KL,
 * nan_to_num(1e6), optimal assignment (exhaustive over <= 8! permutations, first optimum in lexicographic
 * order), loss_b = sum w_i c_i / (sum w_i + 1e-8).  mu, kappa, w (B,maxK); vm_gt (B,maxK,3); K_gt (B) int32.
 * Outputs loss_vec (B), gradients (B,maxK) each, assignment (B,maxK) int32 (-1 beyond K). */
int pnpp_vm_match_loss(const float *mu, const float *kappa, const float *w, const float *vm_gt, const int32_t *K_gt,
                       int B, int maxK, float *loss_vec, float *dmu, float *dkappa, float *dw, int32_t *assign,
                       void *stream);

/* The whole tail of the multi-peak training step in ONE launch: the three output heads o = x [W_pi; W_mu; W_kappa]^T + b
 * (models/pointnet_pp_mvM.py:91-96), the head activations (:91-125), match_loss (train_multi_peaks_vonMises_KL.py:54-81), its batch
 * mean (:229) and their backward.  x (B,K) features; w_pi (max_K,K), w_mu (2 max_K,K), w_kappa (max_K,K); max_K 4 or 8.
 * Writes loss_mean (1), the heads' weight / bias gradients, dx (B,K; may be NULL) and optionally mu, kappa, weight (B,max_K).
 * Bs > 0: the next step's centre draw rides in the same launch (arguments as pnpp_sample_random_dev2); Bs = 0: none. */
int pnpp_mvm_fc_head_match_step(const float *x, const float *w_pi, const float *b_pi, const float *w_mu, const float *b_mu,
                                const float *w_kappa, const float *b_kappa, const float *vm_gt, const int32_t *K_gt, int B, int K,
                                int maxK, float temp, float kappa_max, float *loss_mean, float *dw_pi, float *db_pi, float *dw_mu,
                                float *db_mu, float *dw_kappa, float *db_kappa, float *dx, float *mu, float *kappa, float *weight,
                                uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int Bs, int N1, int npoint1, int32_t *out1,
                                int N2, int npoint2, int32_t *out2, void *stream);
/* pointnet_pp_mvM.py:91-125: raw head outputs -> (mu, kappa, weight) and the backward of that map.
 * pi_raw (B,K), mu_raw (B,2K), kappa_raw (B,K). */
int pnpp_mvm_head(const float *pi_raw, const float *mu_raw, const float *kappa_raw, int B, int K, float temp,
                  float kappa_max, float *mu, float *kappa, float *weight, void *stream);
int pnpp_mvm_head_bwd(const float *pi_raw, const float *mu_raw, const float *kappa_raw, const float *weight,
                      const float *dmu, const float *dkappa, const float *dweight, int B, int K, float temp,
                      float kappa_max, float *dpi_raw, float *dmu_raw, float *dkappa_raw, void *stream);

/* Mixture KL on the decode grid (csrc/mixture_loss_kernels.hip; additive to ABI 5): an objective on the WHOLE predicted mixture.
 *   q(t) = sum_{j < K_gt} v_j vM(t; nu_j, lambda_j)   rows (nu, lambda, v) of vm_gt (B,maxK,3), v normalised by its sum over j < K_gt
 *   p(t) = sum_{i < maxK} w_i vM(t; mu_i, kappa_i)    every predicted component, weights as given
 *   loss_b = (2 pi / G) sum_g q(t_g) (log q(t_g) - log p(t_g)),   t_g = 2 pi g / G,  G = num - 1,  2 <= G <= 1024
 * float64 inside, log-sum-exp over the components, so finite for every kappa <= 500; components of weight <= 0 are skipped; kappa is
 * clamped into [0, 500] and a clamped value gets zero gradient; K_gt <= 0 or sum v <= 0: loss 0, zero gradients; K_gt > maxK is
 * clamped.  mu, kappa, weight (B,maxK), 1 <= maxK <= 8; K_gt (B) int32.  loss_vec (B); dmu, dkappa, dweight (B,maxK) = d loss_b / d.,
 * all three or none (NULL: evaluation only).  One launch, one workgroup per sample, no atomics: two calls are bit-identical. */
int pnpp_mvm_grid_kl(const float *mu, const float *kappa, const float *weight, const float *vm_gt, const int32_t *K_gt, int B, int maxK,
                     int num, float *loss_vec, float *dmu, float *dkappa, float *dweight, void *stream);
/* The same kernel with the multi-peak head inside: pnpp_mvm_head in its prologue, pnpp_mvm_head_bwd in its epilogue (the same device
 * functions).  dpi_raw (B,maxK), dmu_raw (B,2 maxK), dkappa_raw (B,maxK): all three or none; mu, kappa, weight (B,maxK): the head's
 * outputs, all three or none. */
int pnpp_mvm_head_grid_kl(const float *pi_raw, const float *mu_raw, const float *kappa_raw, const float *vm_gt, const int32_t *K_gt,
                          int B, int maxK, float temp, float kappa_max, int num, float *loss_vec, float *dpi_raw, float *dmu_raw,
                          float *dkappa_raw, float *mu, float *kappa, float *weight, void *stream);

/* train_8dir_KL.py:60-68: loss_vec[b] = -sum p * log_softmax(logits); dlogits = softmax*sum(p) - p. */
int pnpp_soft_ce(const float *logits, const float *p, int B, int C, float *loss_vec, float *dlogits, void *stream);

/* ------------------------------------------------------------------------------------------
 * Orientation decoding and angular errors (csrc/decode_kernels.hip; additive to ABI 5)
 * ---------------------------------------------------------------------------------------- */

/* The modes of the mixture p(theta) = sum_k w_k exp(kappa_k (cos(theta - mu_k) - 1)) / (2 pi i0e(kappa_k)) of every sample, one
 * launch, one workgroup per sample, float64 inside.  mu, kappa, weight (B,K), 1 <= K <= 8; weight NULL: weight 1, K = 1 (the
 * single-peak model); counts (B) int32 or NULL: the components in use (clamped to 0..K); a negative or NaN kappa counts as 0.
 * Grid: theta_i = i 2 pi / G, G = num - 1 (models/pointnet_pp_mvM.py:135-136, linspace(0, 2 pi, num)[:-1]), 2 <= G <= 1024.
 * density (B,G) or NULL: p_i / (sum_i p_i + 1e-8), what mvm_density_on_grid returns, finite for kappa up to 500.
 * A grid point is a candidate when p_i > p_{i-1} and p_i >= p_{i+1} (circular); each is refined inside [theta_{i-1}, theta_{i+1}] by
 * 8 rounds of value sectioning on 65 equispaced points (first arg-max, clamped to the interior, the two sub-cells around it kept);
 * the mode is the last bracket's midpoint, its height p there.  Modes are sorted by (height descending, angle in [0, 2 pi) ascending),
 * those below rel_height x the top height are dropped, at most K are kept, angles are wrapped to (-pi, pi].
 * modes, heights (B,K): unused slots NaN and 0; n_modes (B) int32; angle (B) or NULL = modes[:, 0] (NaN when n_modes = 0, which is
 * what a flat density gives). */
int pnpp_mvm_decode(const float *mu, const float *kappa, const float *weight, const int32_t *counts, int B, int K, int num,
                    float rel_height, float *modes, float *heights, int32_t *n_modes, float *angle, float *density, void *stream);

/* Angular errors of decoded orientations, in degrees, and their statistics: one single-workgroup launch.
 * modes (B,K), n_modes (B), angle (B): pnpp_mvm_decode's outputs.  Ground truth: mu_gt, kappa_gt (B), or vm_gt (B,Kmax,3) = (mu, kappa,
 * weight) rows with K_gt (B) int32 as pnpp_vm_match_loss takes them -- one of the two forms, the other's pointers NULL.
 *   top1  = min_j |wrap(angle - mu_gt_j)|,   cover = max_j min_m |wrap(mode_m - mu_gt_j)|,   count_ok = (n_modes == K_gt)
 * A sample with K_gt <= 0, with every ground-truth kappa <= 1e-6 (a symmetric class) or with n_modes = 0 has no error: -1 in both.
 * top1, cover (B) float32 and count_ok (B) int32 may each be NULL.
 * acc or NULL: the accumulator, n_labels * PNPP_ORIENT_STRIDE + 1 words of 64 bits, zeroed by the caller before the first call and
 * added to with integer atomics (any order gives the same words).  Label l's block (labels (B) int32, NULL: all 0; a label outside
 * 0..n_labels-1 is clamped) = [histogram of top1 in 0.5 degree bins (PNPP_ORIENT_BINS) | the same of cover | included | excluded |
 * count_ok | sum of top1 in micro-degrees | sum of cover in micro-degrees | 3 spare]; the last word counts the samples seen.
 * sample_err (capacity,2) or NULL: sample i's (top1, cover) at row (samples seen before this call) + i; rows beyond capacity are
 * dropped and still counted. */
#define PNPP_ORIENT_BINS 360
#define PNPP_ORIENT_STRIDE 728
#define PNPP_ORIENT_MAX_LABELS 64
int pnpp_orient_eval(const float *modes, const int32_t *n_modes, const float *angle, int B, int K, const float *mu_gt,
                     const float *kappa_gt, const float *vm_gt, const int32_t *K_gt, int Kmax, const int32_t *labels, int n_labels,
                     uint64_t *acc, float *sample_err, int64_t capacity, float *top1, float *cover, int32_t *count_ok, void *stream);

/* Classification head of PointNet++Demo.py (csrc/cls_loss_kernels.hip; additive to ABI 5).  One wave per row, any C; the row maximum
 * and the sums are wave reductions, sums in float64.
 * PointNet++Demo.py:234 F.log_softmax(x, dim=1): y (M,C) = x - logsumexp(x, 1);  backward dx = dy - exp(y) * sum_c dy. */
int pnpp_log_softmax(const float *x, int M, int C, float *y, void *stream);
int pnpp_log_softmax_bwd(const float *y, const float *dy, int M, int C, float *dx, void *stream);
/* forward-only tail of the classifier's Predictor, one launch: y (M,C) = log_softmax(x (M,K) w (C,K)^T + b), C <= 1024 */
int pnpp_linear_log_softmax(const float *x, const float *w, const float *b, int M, int K, int C, float *y, void *stream);
/* PointNet++Demo.py:244 F.nll_loss(pred, target) with its default mean reduction: loss_mean[0] = -(1/M) sum_m logp[m, target[m]].
 * target (M) int32 on the device.  A target outside [0, C) adds nothing to the sum and is counted in bad_targets[0] (device int32,
 * always written); there is no ignore_index.  check != 0: the call waits for the stream, reads the count and returns PNPP_ERR_RANGE
 * when it is not zero; check == 0 leaves reading it to the caller (stream capture).  Nothing in the kernel can abort the process.
 * Backward: dlogp (M,C) = -grad_loss[0] / M at the target's column, 0 elsewhere; grad_loss is a device scalar. */
int pnpp_nll_loss(const float *logp, const int32_t *target, int M, int C, float *loss_mean, int32_t *bad_targets, int check, void *stream);
int pnpp_nll_loss_bwd(const int32_t *target, const float *grad_loss, int M, int C, float *dlogp, void *stream);

/* Heads and losses of the other set-abstraction models.
 * models/pointnet_pp_Fwd.py:98, models/Pointnet_pp_xyz.py:84-85, models/Pointnet_pp_xyz_Schedmit.py:87-88:
 * F.normalize(x, p=2, dim=1, eps): y[m,:] = x[m,:] / max(||x[m,:]||, eps); x, y (M,C), C <= 64. */
int pnpp_l2_normalize(const float *x, int M, int C, float eps, float *y, void *stream);
int pnpp_l2_normalize_bwd(const float *x, const float *dy, int M, int C, float eps, float *dx, void *stream);
/* nn.MSELoss() (train.py:168,183; train_multi_8dir.py:80,100; train_8dir.py:53,67): loss[0] = mean_i (p_i - t_i)^2 over
 * all n elements, dp (optional) = 2 (p - t) / n.  One workgroup, fixed-order float64 sum. */
int pnpp_mse(const float *p, const float *t, size_t n, float *loss, float *dp, void *stream);
/* simple_pointnet_train.py:153,174,182: the per-sample form, loss_vec[b] = mean_c (p[b,c] - t[b,c])^2 (its mean over b is
 * nn.MSELoss() of the batch); dp (optional) [b,c] = 2 (p - t) / C. */
int pnpp_mse_rows(const float *p, const float *t, int B, int C, float *loss_vec, float *dp, void *stream);
/* train.py:184-185: loss[0] = mean_b (a_b . b_b)^2 for two (B,C) sets of axes; da, db optional (both or neither). */
int pnpp_orth_loss(const float *a, const float *b, int B, int C, float *loss, float *da, float *db, void *stream);
/* train_multi_8dir.py:41-44 proj_probs: v = normalize(vec (B,3)); sims = clamp(v dirs^T, min=0) with dirs (D,3), D <= 16;
 * probs (B,D) = sims / clamp(sum_j sims, min=1e-8). */
int pnpp_proj_probs(const float *vec, const float *dirs, int B, int D, float *probs, void *stream);
int pnpp_proj_probs_bwd(const float *vec, const float *dirs, const float *dprobs, int B, int D, float *dvec, void *stream);

/* Point-transformer configuration (models/point_transformer.py:4-20), forward pass.
 * input_proj (nn.Linear with at most 8 inputs): y (M,N) = x (M,K) w^T (N,K) + b. */
int pnpp_linear_smallk(const float *x, const float *w, const float *b, int M, int K, int N, float *y, void *stream);
/* nn.MultiheadAttention core (torch.nn.functional.multi_head_attention_forward between in_proj and out_proj):
 * qkv (B,N,3E) with the in_proj bias added, E = H*head_dim, head h = columns h*head_dim.. of each third;
 * out (B,N,E) = concat_h dropout(softmax(q_h k_h^T / sqrt(head_dim))) v_h; lse (B,H,N) optional log-sum-exp of the
 * scaled scores.  The N x N matrix is never materialised.  head_dim must be 16.  N is the number of ROWS per cloud in
 * qkv / out and must be a multiple of 128; the first n_valid of them are points, the rest padding supplied by the caller:
 * keys >= n_valid get no attention weight, outputs of queries >= n_valid are unspecified (finite) and must be ignored
 * (the reference takes any N: models/point_transformer.py:15-20; the drop-in module pads to the next multiple of 128).
 * Dropout on the attention weights (train mode, nn.MultiheadAttention(dropout=p)): mask = bit-packed keep bits from
 * pnpp_attention_dropout_mask (kept weights are scaled by 1/(1-p)); mask == NULL means no dropout (p is then ignored). */
int pnpp_attention_fwd(const float *qkv, int B, int N, int n_valid, int H, int head_dim, const uint32_t *mask, float p,
                       float *out, float *lse, void *stream);
/* Keep bits, Bernoulli(1-p), a pure function of (seed, stream_id, element): mask (B,H,N,N/32) holds for every query the
 * bits of its keys (bit = key % 32 of word key / 32); maskT (B,H,N,N/32) is the transpose (for every key the bits of the
 * queries), read by the dK/dV kernel. */
int pnpp_attention_dropout_mask(uint64_t seed, uint64_t stream_id, int B, int N, int H, float p, uint32_t *mask,
                                uint32_t *maskT, void *stream);
/* The same with the stream id kept in device memory (stream_id_dev[0] = calls so far, stream_id_dev[1] = ticket word, both
 * zero-initialised by the caller): stream id = offset + stream_id_dev[0], read by the launch, which then adds 1 -- a
 * train step captured in a hipGraph draws fresh masks on every replay (nn.Dropout semantics), reproducibly. */
int pnpp_attention_dropout_mask_dev(uint64_t seed, uint64_t *stream_id_dev, uint64_t offset, int B, int N, int H, float p,
                                    uint32_t *mask, uint32_t *maskT, void *stream);
/* Post-norm residual block: y (M,E) = LayerNorm(x + r) * w + b over the last dimension (r may be NULL), E <= 128. */
int pnpp_add_layernorm(const float *x, const float *r, const float *w, const float *b, int M, int E, float eps, float *y,
                       void *stream);
/* x.mean(dim=1): y (B,E) = mean over the N points of x (B,N,E). */
int pnpp_mean_points(const float *x, int B, int N, int E, float *y, void *stream);
/* Backward passes of the four entries above (what torch.autograd derives for the reference model).
 * linear_smallk: dw (N,K) = dy^T x, db (N) = column sums of dy (db may be NULL); x is data, no dx. */
size_t pnpp_linear_smallk_bwd_scratch_bytes(int M, int N);
int pnpp_linear_smallk_bwd(const float *x, const float *dy, int M, int K, int N, float *dw, float *db, void *scratch,
                           void *stream);
/* attention: dqkv (B,N,3E) from qkv, the forward's out and lse, and d_out (B,N,E); dsum (B,H,N) is scratch
 * (rowsum(d_out * out) per head).  Scores are recomputed, never stored.  mask / maskT / p as in the forward (both NULL:
 * no dropout).  n_valid as in the forward: d_out rows >= n_valid must be zero; dK / dV rows >= n_valid are written as zeros. */
int pnpp_attention_bwd(const float *qkv, const float *out, const float *d_out, const float *lse, int B, int N, int n_valid, int H,
                       int head_dim, const uint32_t *mask, const uint32_t *maskT, float p, float *dqkv, float *dsum,
                       void *stream);
/* add_layernorm: du (M,E) = gradient w.r.t. both x and r; dwb (2,E) = (d weight, d bias). */
size_t pnpp_add_layernorm_bwd_scratch_bytes(int M, int E);
int pnpp_add_layernorm_bwd(const float *x, const float *r, const float *w, const float *dy, int M, int E, float eps,
                           float *du, float *dwb, void *scratch, void *stream);
int pnpp_mean_points_bwd(const float *dy, int B, int N, int E, float *dx, void *stream);

/* ------------------------------------------------------------------------------------------
 * Throughput mode of the grouped layers (BASELINE.json configs[1] names a bf16 mode; the reference itself is float32,
 * models/pointnet_pp_8dir.py:40-42): bf16_operands != 0 makes the large 1x1-conv GEMMs of pnpp_sa_forward / pnpp_sa_backward
 * round their two MFMA operands to bfloat16 (float32 accumulate; activations, statistics, transforms stay float32 / float64).
 * Process-wide, default 0 (exact float32), initial value from the environment variable PNPP_MATMUL=bf16.
 * ---------------------------------------------------------------------------------------- */
int pnpp_set_matmul_precision(int bf16_operands);
int pnpp_get_matmul_precision(void);

/* ------------------------------------------------------------------------------------------
 * How the float32 products of the grouped layers' large GEMMs are formed (ABI 5).  0: v_mfma_f32_32x32x2_f32.  1: on the bf16
 * matrix pipe from EXACT three-way operand splits (a float32 is the sum of three bfloat16 numbers; six bf16 x bf16 products per
 * float32 product, each exact in float32, float32 accumulation; the three products dropped are below 2^-25 of the product, i.e.
 * below the rounding of the accumulation): float32 results to float32 rounding -- held to the same parity gates as mode 0 --
 * at 2.67 x the float32 MFMA rate (csrc/gemm_wsf3_kernels.hip).  Not a reduced-precision mode and unrelated to
 * pnpp_set_matmul_precision (which rounds operands to ONE bf16).  Process-wide; initial value from PNPP_SPLIT_PRODUCTS.
 * ---------------------------------------------------------------------------------------- */
int pnpp_set_split_products(int on);
int pnpp_get_split_products(void);

/* ------------------------------------------------------------------------------------------
 * How the large kernels' stores leave the chip: a mask of site classes whose stores are write-through (sc1: the bytes go to memory as
 * they are stored) instead of plain write-back (the lines stay dirty in the writing XCD's L2 until the launch ends).
 *   1  dW partial slabs (read next by post_gemm / slab_reduce / xyz0_post)
 *   2  float64 statistics slabs and moment partials
 *   4  streamed activation and gradient outputs of the fused GEMMs
 * Values and order of every store are the same under every mask: results are bit-identical (tests/test_gpu_store_policy.py).
 * Process-wide, default 5 (classes 1 and 4: the ones that measured faster on the training step); no environment variable.  A hipGraph captured under one mask keeps it.  A mask with other bits is
 * PNPP_ERR_ARG.
 * ---------------------------------------------------------------------------------------- */
int pnpp_set_store_policy(int mask);
int pnpp_get_store_policy(void);
/* diagnostics: non-zero once a bounded LDS poll of the wave-pair kernel (csrc/gemm_wsd3_kernels.hip) has given up in this process */
int pnpp_debug_wsd3_timeouts(void);

/* ------------------------------------------------------------------------------------------
 * SyncBN (ABI 3; off by default): cross-rank exchange of the train-mode BatchNorm sums under data parallelism, so that a
 * global batch split over ranks normalises exactly like the reference's single process on the concatenated batch
 * (nn.BatchNorm2d / nn.BatchNorm1d in training mode: models/pointnet_pp_8dir.py:40-41, models/pointnet_pp_vonMises.py:32-33).
 * Once a callback is registered, every training-mode BatchNorm of pnpp_sa_forward / pnpp_sa_backward / pnpp_fc_forward /
 * pnpp_fc_backward reduces this rank's per-channel sums -- forward (sum z, sum z^2, rows), backward (sum dy, sum dy*xhat, rows) --
 * into buf[0 .. 2C], calls fn(buf, 2C + 1, stream, user), which must replace those doubles by their SUM OVER ALL RANKS,
 * stream-ordered behind `stream` (RCCL: an all-reduce enqueued on it; gloo: a blocking all-reduce), and finalises from the
 * summed values.  Parameter gradients of the BatchNorm layers stay rank-local sums (the gradient all-reduce adds them up like
 * every other parameter's); running statistics become the global ones on every rank.  buf: caller-owned device memory of
 * buf_doubles >= 2 * (2 * C_max + 1) doubles (second half: the rank's own sums).  fn == NULL unregisters.
 * The head's fused BatchNorm epilogue and its in-kernel dropout draw need the whole batch in one tile and are bypassed while a
 * callback is registered (pass an explicit mask).  Process-wide, like the matmul precision.
 * ---------------------------------------------------------------------------------------- */
typedef int (*pnpp_stats_exchange_fn)(double *buf, size_t n_doubles, void *stream, void *user);
int pnpp_set_stats_exchange(pnpp_stats_exchange_fn fn, void *user, double *buf, size_t buf_doubles);
int pnpp_stats_exchange_enabled(void);

/* ------------------------------------------------------------------------------------------
 * Vanilla PointNet (models/pointnet.py; additive to ABI 5).  float32 products whatever pnpp_set_matmul_precision /
 * pnpp_set_split_products say; statistics and reductions over points in float64; no float atomics (bitwise replay).
 * The training-mode entry points return PNPP_ERR_ARG while a statistics exchange (SyncBN) is registered.
 *
 * Sizes: B <= 65535 (clouds are a grid dimension).
 * Pooled wide layer: out[b, c] = max over the cloud's N rows of act(BN(A W^T + b))[n, c], A = (B*N, K) rows.  Nothing of size
 * (B*N) x C is stored: the forward pass keeps the cloud's max / min of z = A W^T + b per channel and its row (first on ties), the
 * training statistics come from the column sums and the Gram matrix of A; the backward pass is one (B*N) x K x K product plus
 * a routed scatter ("Vanilla PointNet").
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int B, N;            /* clouds, points per cloud                                                      */
    int K, C;            /* input width (multiple of 4, <= 128), channels (multiple of 64, <= 1024)        */
    int relu;            /* ReLU after the BatchNorm (the T-Nets' conv3) or none (the encoder's conv3)     */
    int training;        /* batch statistics + running update, or the running statistics                  */
    float eps, momentum;
} pnpp_pn_pool_desc;

typedef struct {
    const float *a;      /* (B*N, K), 16-byte aligned                                                     */
    const float *w, *b;  /* (C, K), (C)                                                                   */
    const float *gamma, *beta;
    float *rm, *rv;      /* running statistics (C), updated in training                                   */
    int64_t *nbt;        /* num_batches_tracked (+1 in training) or NULL                                   */
    float *out;          /* (B, C)                                                                        */
    void *saved;         /* pnpp_pn_pool_saved_bytes()                                                    */
    void *scratch;       /* pnpp_pn_pool_scratch_bytes()                                                  */
} pnpp_pn_pool_fwd_args;

typedef struct {
    const float *a, *w, *gamma;
    const float *dout;   /* (B, C)                                                                        */
    const void *saved;
    void *scratch;
    float *da;           /* (B*N, K) or NULL                                                              */
    float *dw, *db, *dgamma, *dbeta;  /* db is 0 in training (the BatchNorm removes the bias)               */
} pnpp_pn_pool_bwd_args;

size_t pnpp_pn_pool_saved_bytes(const pnpp_pn_pool_desc *d);     /* 0: bad descriptor (pnpp_last_error) */
size_t pnpp_pn_pool_scratch_bytes(const pnpp_pn_pool_desc *d);
int pnpp_pn_pool_forward(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_fwd_args *a, void *stream);
int pnpp_pn_pool_backward(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_bwd_args *a, void *stream);
/* diagnostics: views into a forward call's saved workspace -- the (B, C) int32 row each pooled value came from (its max route,
 * local to the cloud) and the (B, C) float32 z at that row */
void *pnpp_pn_pool_saved_route(const pnpp_pn_pool_desc *d, void *saved);
void *pnpp_pn_pool_saved_zsel(const pnpp_pn_pool_desc *d, void *saved);
/* ... and the (B, C) float32 pre-activation act() was applied to: with relu, the ReLU decision at the pooled value is ypre > 0 */
void *pnpp_pn_pool_saved_ypre(const pnpp_pn_pool_desc *d, void *saved);

/* Per-cloud transform: y[b, n, j] = sum_i x[b, n, i] t[b, i, j] for j < k, x[b, n, j] for k <= j < D, 0 for D <= j < ldy;
 * x element (b, n, d) at x[b*sb + n*sn + d*sd] (so (B, D, N) and (B, N, D) inputs are both read in place), y (B*N, ldy) rows.
 * t == NULL: no product (a strided copy into padded rows).  D <= 64, k <= D, D <= ldy <= 64.
 * Backward: dx (x's strides, D columns) = dy t^T on the transformed columns, dy on the others; dt[b] = x_b^T dy_b over the cloud's
 * points in float64, fixed order.  dx / dt may be NULL. */
int pnpp_pn_transform(const float *x, int64_t sb, int64_t sn, int64_t sd, const float *t, int B, int N, int D, int k, int ldy,
                      float *y, void *stream);
int pnpp_pn_transform_bwd(const float *x, int64_t sb, int64_t sn, int64_t sd, const float *t, const float *dy, int B, int N, int D,
                          int k, int ldy, float *dx, float *dt, void *stream);
/* feature-transform regulariser out[0] = mean_b ||t_b t_b^T - I||_F, norms (B doubles, caller-owned) kept for the backward pass;
 * backward: dt_b = dout[0] * 2 (t_b t_b^T - I) t_b / (B ||.||_F) (0 where the norm is 0) */
int pnpp_pn_regularizer(const float *t, int B, int k, double *norms, float *out, void *stream);
int pnpp_pn_regularizer_bwd(const float *t, const double *norms, const float *dout, int B, int k, float *dt, void *stream);
/* y = x + I per cloud (the T-Nets' "fc3 + iden"); its backward is the identity */
int pnpp_pn_add_identity(const float *x, int B, int k, float *y, void *stream);
/* out (B, C1 + C2, N) = [g repeated over the points; pf (B*N, C2) rows transposed] and its backward (dg: sum over the points) */
int pnpp_pn_concat(const float *g, const float *pf, int B, int N, int C1, int C2, float *out, void *stream);
int pnpp_pn_concat_bwd(const float *dout, int B, int N, int C1, int C2, float *dg, float *dpf, void *stream);
/* relu(BatchNorm1d(x)) over (M, C) rows on its own -- the PointNet head's relu(bn2(dropout(fc2(x)))); mean / istd (C) kept for
 * the backward pass, which reads the forward output y for the ReLU decisions.  dx may be NULL. */
int pnpp_pn_bn_relu(const float *x, int M, int C, const float *gamma, const float *beta, float *rm, float *rv, int64_t *nbt,
                    int training, float eps, float momentum, float *mean, float *istd, float *y, void *stream);
int pnpp_pn_bn_relu_bwd(const float *x, const float *y, const float *dy, int M, int C, const float *gamma, const float *mean,
                        const float *istd, int training, float *dx, float *dgamma, float *dbeta, void *stream);

/* Ragged batches (additive to ABI 5): cloud b holds the first len_b of its N padded points, 1 <= len_b <= N.  The valid point rows
 * are PACKED, cloud after cloud: offs (B + 1) int32 on the device is the exclusive prefix sum of the lengths, row n of cloud b is
 * packed row offs[b] + n, and M_total = offs[B] = sum of the lengths is the row count of every packed (M_total, width) array (A, dA,
 * the transforms' y / dy, the concat's pf / dpf).  Padded arrays keep their (B, N) addressing; what they hold at n >= len_b is
 * never read (NaN included), and what is written there is an exact 0.  The BatchNorm statistics of the pooled layer run over the
 * M_total packed rows (running variance scaled by M_total / (M_total - 1)), each cloud's max and its route (still local to the cloud)
 * over its own rows.  Descriptors, argument structs and workspace layouts are those of the namesakes; d->N is the padded N, which
 * sizes the grids and the Gram slices, so offs == {0, N, 2N, ...} reproduces the uniform call bit for bit.
 *   pnpp_pn_pool_*_ragged        M_total in [B, B*N], > 1 when training
 *   pnpp_pn_transform*_ragged    x_packed == 0: x / dx are the padded strided input (dx zero at padding); x_packed == 1: x / dx are
 *                                packed rows of pitch sn themselves (sb unused): the feature transform of an already packed layer
 *   pnpp_pn_concat_ragged        pf_padded == 1: pf has the padded B*N rows (the tapped rows of pnpp_pn_infer_ragged)
 *   pnpp_pn_concat_bwd_ragged    dout at padding columns is not read; dpf packed
 *   pnpp_pn_infer_ragged         x and feat_out padded (feat_out rows n >= len_b zero); out[b] bit-equal to the call on cloud b alone */
/* lengths (B) int32 on the device -> lens_out (B) = min(max(lengths[b], 1), N) and offs (B + 1), their exclusive prefix sum: one
 * small launch, no synchronisation (a host that knows the lengths writes both arrays itself) */
int pnpp_pn_offsets(const int32_t *lengths, int B, int N, int32_t *lens_out, int32_t *offs, void *stream);
size_t pnpp_pn_pool_saved_bytes_ragged(const pnpp_pn_pool_desc *d, int M_total);
size_t pnpp_pn_pool_scratch_bytes_ragged(const pnpp_pn_pool_desc *d, int M_total);
int pnpp_pn_pool_forward_ragged(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_fwd_args *a, const int32_t *offs, int M_total, void *stream);
int pnpp_pn_pool_backward_ragged(const pnpp_pn_pool_desc *d, const pnpp_pn_pool_bwd_args *a, const int32_t *offs, int M_total,
                                 void *stream);
int pnpp_pn_transform_ragged(const float *x, int x_packed, int64_t sb, int64_t sn, int64_t sd, const float *t, const int32_t *offs, int B,
                             int N, int D, int k, int ldy, float *y, void *stream);
int pnpp_pn_transform_bwd_ragged(const float *x, int x_packed, int64_t sb, int64_t sn, int64_t sd, const float *t, const float *dy,
                                 const int32_t *offs, int B, int N, int D, int k, int ldy, float *dx, float *dt, void *stream);
int pnpp_pn_concat_ragged(const float *g, const float *pf, int pf_padded, const int32_t *offs, int B, int N, int C1, int C2, float *out,
                          void *stream);
int pnpp_pn_concat_bwd_ragged(const float *dout, const int32_t *offs, int B, int N, int C1, int C2, float *dg, float *dpf, void *stream);

/* ------------------------------------------------------------------------------------------
 * Forward-only (inference) path of the set-abstraction levels (additive to ABI 5; csrc/sa_infer_kernels.hip).
 * models/pointnet_pp_8dir.py:21-43 with the BatchNorms in eval mode: running statistics make each BatchNorm an affine map,
 * which is folded into the convolution in front of it ONCE (pnpp_sa_infer_fold, float64 rounded once to float32):
 *     a = gamma / sqrt(running_var + eps),  W' = a (.) W row-wise,  b' = (b - running_mean) * a + beta.
 * A level is then ONE launch: gather -> 3 x (product + b' + ReLU) -> max over the neighbourhood; the intermediate M x C tiles
 * stay in LDS / registers, only (B,S,C_last) and new_xyz are written.  No backward pass exists for this path, there is no
 * `saved` and no `scratch`: pnpp_sa_forward with training = 0 remains the differentiable eval path and the path for every other shape.
 *
 * Shapes the fused kernel takes (pnpp_sa_infer_supported answers for a descriptor; d->training and d->momentum are ignored):
 *   L == 3;  every C[l] a multiple of 32, at most 1024;  K == 16 or a multiple of 32 up to 256 (group_all: N likewise);  D <= 1021;
 *   (K > 32: a workgroup owns one neighbourhood and walks it in 32-row tiles, the running column maximum stays in registers);
 *   a 32-row tile of widths max(round16(D+3), C[1]) + 8 and C[0] + 8, three bfloat16 planes each, must fit 160 KiB of LDS;  any B, N, S within int32 sizes.
 * float32 products formed on the bf16 matrix pipe from exact three-way operand splits (the arithmetic pnpp_set_split_products(1)
 * describes: float32 results to float32 rounding, same parity gates) whatever pnpp_set_matmul_precision / pnpp_set_split_products say;
 * the weights' planes are written once by pnpp_sa_infer_fold, an activation is split once where it is produced.
 *
 * The folded-parameter blob (pnpp_sa_infer_weights_bytes, caller-owned device memory) holds per layer W'_l (C[l] x ld_l, xyz columns
 * first, zeros beyond the layer's input width; ld_0 = D + 3 rounded up to 16, ld_l = C[l-1]) and b'_l (C[l], float32).  W'_l is stored
 * as the THREE bfloat16 planes of its exact three-way split (W' = high + middle + low, 8 + 8 + 8 significand bits: the operands of the
 * split products below), each C[l] * ld_l elements, one after the other, each in the order the kernel's lanes read it
 * ("fragment-major"): element (n, k) of a plane at bf16 index
 *     (((n / 32) * (ld_l / 16) + k / 16) * 64 + 32 * ((k % 16) / 8) + n % 32) * 8 + k % 8,
 * i.e. the blob holds [3][C/32][ld/16][2][32][8] bfloat16 per layer.  pnpp_sa_infer_weights_layout gives the byte offsets and ld_l of a layer (the documented
 * view the parity tests read back).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    const float *xyz;             /* (B,N,3)                                                                          */
    const float *points;          /* (B,N,D) or NULL                                                                  */
    const int32_t *centre_idx;    /* (B,S) centre indices (unused when group_all)                                     */
    const int32_t *neighbour_idx; /* (B,S,K) neighbours (ball query, injection), or NULL: the level searches kNN itself */
    int32_t *idx_out;             /* (B,S,K) caller-owned; receives the kNN result when neighbour_idx is NULL         */
    const void *weights;          /* blob written by pnpp_sa_infer_fold for the same descriptor                       */
    float *new_xyz;               /* out (B,S,3): the gathered centres, zeros when group_all                          */
    float *out;                   /* out (B,S,C[2])                                                                   */
} pnpp_sa_infer_args;

/* 1: the fused kernel takes the shape.  0: it does not, pnpp_last_error() names the reason */
int pnpp_sa_infer_supported(const pnpp_sa_desc *d);
/* bytes of the folded-parameter blob; 0 for a refused descriptor */
size_t pnpp_sa_infer_weights_bytes(const pnpp_sa_desc *d);
int pnpp_sa_infer_weights_layout(const pnpp_sa_desc *d, int layer, size_t *w_offset_host, int *w_ld_host, size_t *b_offset_host);
/* reads conv_w / conv_b / bn_w / bn_b / bn_rm / bn_rv of `params` (every other member is ignored, nothing is written to them) and
 * writes the blob: one launch per layer */
int pnpp_sa_infer_fold(const pnpp_sa_desc *d, const pnpp_sa_fwd_args *params, void *weights, void *stream);
int pnpp_sa_infer(const pnpp_sa_desc *d, const pnpp_sa_infer_args *a, void *stream);
/* pnpp_sa_group_pair for this path (models/pointnet_pp_8dir.py:28-31 of sa1 and sa2 in ONE launch): the neighbour indices go to
 * plain (B,S,K) int32 buffers, the centre coordinates to new_xyz1 / new_xyz2; pass idx1 / idx2 as neighbour_idx to pnpp_sa_infer */
int pnpp_sa_infer_group_pair(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *centre1,
                             const int32_t *centre2, int32_t *idx1, float *new_xyz1, int32_t *idx2, float *new_xyz2, void *stream);
/* ... of a ragged batch: lengths (B) int32 on the device, level 1's clouds (see pnpp_sa_group_pair_ragged) */
int pnpp_sa_infer_group_pair_ragged(const pnpp_sa_desc *d1, const pnpp_sa_desc *d2, const float *xyz, const int32_t *lengths,
                                    const int32_t *centre1, const int32_t *centre2, int32_t *idx1, float *new_xyz1, int32_t *idx2,
                                    float *new_xyz2, void *stream);
/* The same fold for a head block, nn.Linear (N,K) + eval-mode nn.BatchNorm1d (models/pointnet_pp_vonMises.py:32-33,
 * pointnet_pp_8dir.py:81-84): w_out (N,K), b_out (N).  The folded block then runs as pnpp_fc_forward with norm = PNPP_NORM_NONE,
 * training = 0 on (w_out, b_out): y = relu(x W'^T + b'). */
int pnpp_fc_infer_fold(int N, int K, const float *w, const float *b, const float *gamma, const float *beta, const float *rm,
                       const float *rv, float eps, float *w_out, float *b_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Forward-only (inference) path of a vanilla PointNet trunk (additive to ABI 5; csrc/pointnet_infer_kernels.hip).
 * A trunk of models/pointnet.py in eval mode is a chain of per-point layers (1x1 convolution + BatchNorm, folded as above) followed
 * by a max over the cloud's N points.  ONE launch runs the chain on row tiles that stay in LDS / registers and takes the max on the
 * last layer's accumulators; a small second launch finishes the max over a cloud's row slices, adds b' and applies the ReLU
 * (monotone, so after the max).  Nothing of size B*N x C is written for C > 64.
 *   rows        x[b, n, :D] read through element strides (either input layout), zero-padded to a multiple of 16 columns;
 *   input_transform: the first three columns are multiplied by the cloud's 3 x 3 matrix `trans` while the operand is built;
 *   layers      L = 2 .. 4, widths C[l] multiples of 32 up to 1024, ReLU after every layer but the last, where relu_last decides;
 *   transform_after = l >= 0: layer l's output (C[l] == 64) is multiplied by the cloud's 64 x 64 matrix `trans_feat` before layer
 *                 l + 1 (a product layer of its own inside the kernel; its planes are split per call by a small launch); -1: none.
 * Products, planes and the blob layout are those of pnpp_sa_infer (ld_0 = D rounded up to 16, ld_l = C[l-1]); any B >= 1, N >= 1.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int B, N;                 /* clouds, points per cloud                                                             */
    int D;                    /* input columns per point (the first layer's input channels)                           */
    int L;                    /* layers, 2 .. PNPP_MAX_LAYERS                                                         */
    int C[PNPP_MAX_LAYERS];   /* their widths                                                                         */
    int input_transform;      /* 1: x[..., :3] @ trans[b] while the layer-0 operand is built (D >= 3)                 */
    int transform_after;      /* layer whose output is multiplied by trans_feat[b] (C[l] == 64, l < L - 1), or -1     */
    int relu_last;            /* ReLU on the pooled layer (the T-Nets) or not (the encoder)                           */
    float eps;                /* of the BatchNorms (pnpp_pn_infer_fold)                                               */
} pnpp_pn_infer_desc;

typedef struct {
    const float *x;               /* element (b, n, c) at x[b * stride_b + n * stride_n + c * stride_c]                */
    int64_t stride_b, stride_n, stride_c;
    const float *trans;           /* (B,3,3), with input_transform                                                     */
    const float *trans_feat;      /* (B,64,64), with transform_after >= 0                                              */
    const void *weights;          /* blob written by pnpp_pn_infer_fold for the same layers                            */
    void *scratch;                /* pnpp_pn_infer_scratch_bytes: partial maxima, the planes of trans_feat             */
    float *out;                   /* out (B, C[L-1])                                                                   */
    float *feat_out;              /* optional out (B*N, C[feat_layer]): layer feat_layer's output rows (after trans_feat when it
                                     applies there); only for a 64-wide layer (PointNetEncoder(global_feat=False))     */
    int feat_layer;
} pnpp_pn_infer_args;

/* 1: the fused kernel takes the trunk.  0: it does not, pnpp_last_error() names the reason */
int pnpp_pn_infer_supported(const pnpp_pn_infer_desc *d);
/* bytes of the folded-parameter blob (independent of B and N); 0 for a refused descriptor */
size_t pnpp_pn_infer_weights_bytes(const pnpp_pn_infer_desc *d);
int pnpp_pn_infer_weights_layout(const pnpp_pn_infer_desc *d, int layer, size_t *w_offset_host, int *w_ld_host, size_t *b_offset_host);
/* bytes of the per-call workspace at the descriptor's B and N: O(B * slices * C[L-1]) partial maxima + B * 24 KiB of planes with
 * transform_after; 0 for a refused descriptor */
size_t pnpp_pn_infer_scratch_bytes(const pnpp_pn_infer_desc *d);
/* reads conv_w / conv_b / bn_w / bn_b / bn_rm / bn_rv [0 .. L) of `params` (every other member is ignored) and writes the blob */
int pnpp_pn_infer_fold(const pnpp_pn_infer_desc *d, const pnpp_sa_fwd_args *params, void *weights, void *stream);
int pnpp_pn_infer(const pnpp_pn_infer_desc *d, const pnpp_pn_infer_args *a, void *stream);
/* ... of a ragged batch (offs as for pnpp_pn_pool_forward_ragged; d->N the padded N, which sizes the scratch) */
int pnpp_pn_infer_ragged(const pnpp_pn_infer_desc *d, const pnpp_pn_infer_args *a, const int32_t *offs, void *stream);

/* ------------------------------------------------------------------------------------------
 * Forward-only (inference) path of the point transformer (additive to ABI 5; csrc/transformer_infer_kernels.hip).
 * models/point_transformer.py in eval mode: everything of an encoder layer behind the attention is row-local, so a forward is
 *     pnpp_pt_infer_head                         x0 = xyz W_p^T + b_p,  qkv_0 = x0 W_in^T + b_in
 *     depth x ( pnpp_attention_infer or pnpp_attention_fwd (lse = NULL), pnpp_pt_infer_tail )
 *     pnpp_pt_infer_pool                         mean over the cloud's n_valid points, fc_out
 * = 2 + 2 * depth launches.  A tail launch computes, per 32-row tile,
 *     u = LN1(x + o W_out^T + b_out);  y = LN2(u + relu(u W_1^T + b_1) W_2^T + b_2) -> x_next;
 *     qkv_next = y W_in'^T + b_in' (the next layer's in_proj), or in the last layer the tile's column sums over its rows < n_valid;
 * the F-wide hidden activation is produced and consumed 64 columns at a time and never leaves the chip.  Products, planes and the
 * fragment-major layout [3][C/32][ld/16][2][32][8] are those of pnpp_sa_infer.
 * Shapes taken (pnpp_pt_infer_supported): E == 64, H == 4 (head dimension 16), F a multiple of 64, 1 <= in_dim <= 8, N (rows per cloud)
 * a multiple of 128 with 1 <= n_valid <= N points (the caller pads: rows >= n_valid are computed as zero points and never pooled);
 * the post-norm, ReLU, packed in_proj, batch_first encoder layer with biases.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int B, N;                 /* clouds, rows per cloud (a multiple of 128)                                           */
    int n_valid;              /* points per cloud, 1 .. N                                                             */
    int in_dim;               /* input columns per point, 1 .. 8                                                      */
    int E, H, F;              /* embedding, heads, dim_feedforward                                                    */
    int depth;                /* encoder layers                                                                       */
    float eps;                /* of the LayerNorms                                                                    */
} pnpp_pt_infer_desc;

/* device pointers to one encoder layer's float32 parameters, as nn.TransformerEncoderLayer stores them */
typedef struct {
    const float *in_proj_w, *in_proj_b;       /* (3E, E), (3E)  */
    const float *out_proj_w, *out_proj_b;     /* (E, E), (E)    */
    const float *linear1_w, *linear1_b;       /* (F, E), (F)    */
    const float *linear2_w, *linear2_b;       /* (E, F), (E)    */
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;   /* (E) each */
} pnpp_pt_infer_layer_params;

/* matrix index of pnpp_pt_infer_weights_layout */
#define PNPP_PT_IN_PROJ 0
#define PNPP_PT_OUT_PROJ 1
#define PNPP_PT_LINEAR1 2
#define PNPP_PT_LINEAR2 3
#define PNPP_PT_NORM1 4
#define PNPP_PT_NORM2 5
#define PNPP_PT_INPUT_PROJ 6

/* 1: the fused kernels take the shape.  0: they do not, pnpp_last_error() names the field */
int pnpp_pt_infer_supported(const pnpp_pt_infer_desc *d);
/* bytes of ONE LAYER's folded-parameter blob (independent of B, N, n_valid and the layer): a caller holds `depth` of them, so that none
 * of its allocations is larger than a layer's planes; 0 for a refused descriptor */
size_t pnpp_pt_infer_weights_bytes(const pnpp_pt_infer_desc *d);
/* byte offsets inside layer `layer`'s blob (the same for every layer).  matrix 0 .. 3: three bfloat16 planes of rows x ld at w_offset
 * (fragment-major), float32 bias at b_offset.  matrix 4 / 5: norm1 / norm2, float32 weight at w_offset and bias at b_offset, ld = E.
 * matrix 6: input_proj as float32 (E, ld = 8) row-major, zero beyond in_dim, bias at b_offset (written to layer 0's blob only). */
int pnpp_pt_infer_weights_layout(const pnpp_pt_infer_desc *d, int layer, int matrix, size_t *w_offset_host, int *w_ld_host,
                                 size_t *b_offset_host);
/* writes layer `layer`'s blob from `params` (host struct of device pointers); layer 0 also takes input_proj (E, in_dim), (E) */
int pnpp_pt_infer_fold(const pnpp_pt_infer_desc *d, int layer, const pnpp_pt_infer_layer_params *params, const float *input_w,
                       const float *input_b, void *weights, void *stream);
/* bytes of the last layer's partial sums (B, N/32, E) float32; 0 for a refused descriptor */
size_t pnpp_pt_infer_scratch_bytes(const pnpp_pt_infer_desc *d);
/* xyz (B, n_valid, in_dim) contiguous, unpadded -> x0 (B*N, E), qkv0 (B*N, 3E); weights0: layer 0's blob */
int pnpp_pt_infer_head(const pnpp_pt_infer_desc *d, const float *xyz, const void *weights0, float *x0, float *qkv0, void *stream);
/* layer `layer` (blob `weights`): x, o (B*N, E) -> x_next (B*N, E, not x or o) and qkv_next (B*N, 3E) through the in_proj of the next
 * layer's blob `weights_next`, or for layer == depth - 1 the partial sums in `scratch` (qkv_next and weights_next are ignored there,
 * scratch elsewhere) */
int pnpp_pt_infer_tail(const pnpp_pt_infer_desc *d, int layer, const float *x, const float *o, const void *weights, const void *weights_next,
                       float *x_next, float *qkv_next, void *scratch, void *stream);
/* out (B, n_out) = (sum of the cloud's partial sums / n_valid) fc_w^T + fc_b, fc_w (n_out, E) float32; fixed summation order */
int pnpp_pt_infer_pool(const pnpp_pt_infer_desc *d, const void *scratch, const float *fc_w, const float *fc_b, int n_out, float *out,
                       void *stream);
/* The attention of that path (additive to ABI 5; csrc/attention_infer_kernels.hip): what pnpp_attention_fwd computes with mask == NULL
 * and lse == NULL, on the same qkv (B, N, 3E) and out (B, N, E) buffers and with the same padding contract, both products formed on
 * v_mfma_f32_32x32x16_bf16 from the exact three-way bfloat16 splits of their float32 operands.  No workspace, one launch.
 * Shapes taken: head_dim == 16, N a multiple of 128, 1 <= n_valid <= N, B and H >= 1 (at most 65535 each).  Arguments are validated
 * before anything is launched; for a refused shape pnpp_last_error() names the field. */
int pnpp_attention_infer(const float *qkv, int B, int N, int n_valid, int H, int head_dim, float *out, void *stream);
/* 1: pnpp_attention_infer takes the shape.  0: it does not, pnpp_last_error() names the field */
int pnpp_attention_infer_supported(int B, int N, int n_valid, int H, int head_dim);
/* The TRAINING attention in the same form (additive to ABI 5; csrc/attention_train_kernels.hip).  pnpp_attention_split_fwd mirrors
 * pnpp_attention_fwd and pnpp_attention_split_bwd mirrors pnpp_attention_bwd: the same argument lists, buffers (qkv, mask / maskT, out,
 * lse, d_out, dqkv, dsum), status codes and padding contract (d_out rows >= n_valid zero; rows >= n_valid of dqkv come back as exact
 * zeros; nothing a row < n_valid receives depends on what the padding rows hold), with every matrix product formed on
 * v_mfma_f32_32x32x16_bf16 from the exact three-way bfloat16 splits of its float32 operands.  The softmax denominator, hence lse, is over
 * the undropped weights and does not depend on the mask, bit for bit.  No workspace, no allocation, no host copy, no synchronisation:
 * stream-ordered and capturable; no atomics: repeats are bit-equal.  One launch forward, two backward.  Shapes taken: those of
 * pnpp_attention_infer; arguments are validated before anything is launched. */
int pnpp_attention_split_fwd(const float *qkv, int B, int N, int n_valid, int H, int head_dim, const uint32_t *mask, float p,
                             float *out, float *lse, void *stream);
int pnpp_attention_split_bwd(const float *qkv, const float *out, const float *d_out, const float *lse, int B, int N, int n_valid, int H,
                             int head_dim, const uint32_t *mask, const uint32_t *maskT, float p, float *dqkv, float *dsum,
                             void *stream);
/* 1: the two entries above take the shape.  0: they do not, pnpp_last_error() names the field */
int pnpp_attention_split_supported(int B, int N, int n_valid, int H, int head_dim);

/* Ragged batches of the point transformer (additive to ABI 5): the padded layout stays -- x (B, N rows, ...) -- and `lengths` (B) int32
 * in device memory says how many of cloud b's rows are points: rows 0 .. lengths[b] - 1; the rest of its rows are padding.  Each entry
 * is its namesake with that tensor added, runs the same kernels through the same launch code (the namesake is the call with
 * lengths == NULL) and obeys the same size rules; a null `lengths` is PNPP_ERR_ARG, and every argument is checked before anything is
 * launched.  Inside the kernels a cloud's length is min(max(lengths[b], 1), n_valid): no value in the tensor can cause an access
 * outside the rows the uniform call touches, and the host never reads it (no synchronisation; a captured graph stays valid while the
 * lengths change).  Per cloud b the results are those of the namesake on that cloud alone with n_valid = lengths[b], bit for bit; in
 * addition the rows >= lengths[b] of out and dqkv come back as exact zeros and lse is 0 there, and a 128-row workgroup that lies wholly
 * beyond its cloud does no attention work.  What the padding rows of qkv hold must be finite, as for the namesakes.
 *   pnpp_mean_points_ragged      y[b] = sum_{n < len_b} x[b][n] / len_b, x (B, N, E) read in place at row pitch N
 *   pnpp_mean_points_bwd_ragged  dx[b][n] = dy[b] / len_b for n < len_b, an exact 0 otherwise
 *   pnpp_pt_infer_*_ragged       head: xyz (B, n_valid, in_dim), rows >= len_b are taken as zero points whatever they hold (NaN included);
 *                                tail: the last layer pools rows < len_b only; pool: divides by len_b.  Every row of x_next and qkv_next is
 *                                written on every call, so no stale value of a reused buffer reaches a later kernel. */
int pnpp_attention_fwd_ragged(const float *qkv, int B, int N, int n_valid, const int32_t *lengths, int H, int head_dim, const uint32_t *mask,
                              float p, float *out, float *lse, void *stream);
int pnpp_attention_bwd_ragged(const float *qkv, const float *out, const float *d_out, const float *lse, int B, int N, int n_valid,
                              const int32_t *lengths, int H, int head_dim, const uint32_t *mask, const uint32_t *maskT, float p, float *dqkv,
                              float *dsum, void *stream);
int pnpp_attention_split_fwd_ragged(const float *qkv, int B, int N, int n_valid, const int32_t *lengths, int H, int head_dim,
                                    const uint32_t *mask, float p, float *out, float *lse, void *stream);
int pnpp_attention_split_bwd_ragged(const float *qkv, const float *out, const float *d_out, const float *lse, int B, int N, int n_valid,
                                    const int32_t *lengths, int H, int head_dim, const uint32_t *mask, const uint32_t *maskT, float p,
                                    float *dqkv, float *dsum, void *stream);
int pnpp_attention_infer_ragged(const float *qkv, int B, int N, int n_valid, const int32_t *lengths, int H, int head_dim, float *out,
                                void *stream);
int pnpp_mean_points_ragged(const float *x, int B, int N, const int32_t *lengths, int E, float *y, void *stream);
int pnpp_mean_points_bwd_ragged(const float *dy, int B, int N, const int32_t *lengths, int E, float *dx, void *stream);
int pnpp_pt_infer_head_ragged(const pnpp_pt_infer_desc *d, const int32_t *lengths, const float *xyz, const void *weights0, float *x0,
                              float *qkv0, void *stream);
int pnpp_pt_infer_tail_ragged(const pnpp_pt_infer_desc *d, const int32_t *lengths, int layer, const float *x, const float *o,
                              const void *weights, const void *weights_next, float *x_next, float *qkv_next, void *scratch, void *stream);
int pnpp_pt_infer_pool_ragged(const pnpp_pt_infer_desc *d, const int32_t *lengths, const void *scratch, const float *fc_w, const float *fc_b,
                              int n_out, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Step glue on one flat parameter / gradient buffer (csrc/optim_kernels.hip)
 * (train_single_peak_vonMises_KL.py:80,85; train_multi_peaks_vonMises_KL.py:221,235-236)
 * ---------------------------------------------------------------------------------------- */
/* torch.optim.Adam(lr, betas, eps, weight_decay=0) single fused update; step is 1-based. */
int pnpp_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, int step, float lr,
                   float beta1, float beta2, float eps, float grad_scale, void *stream);
/* The same update, clearing each gradient once it has been consumed: the opt.zero_grad() of the next iteration
 * (train_single_peak_vonMises_KL.py:80) folded into the optimiser launch. */
int pnpp_adam_step_zero(float *param, float *grad, float *exp_avg, float *exp_avg_sq, size_t n, int step, float lr,
                        float beta1, float beta2, float eps, float grad_scale, void *stream);

/* The same update for launches captured in a hipGraph: the step count lives in device memory (step_state[0] = steps
 * taken so far, step_state[1] = ticket word, both zero-initialised by the caller) and is advanced by the launch
 * itself, so every replay applies its own bias correction.  zero_grad != 0 clears each gradient after it has been
 * consumed -- the opt.zero_grad() of the next iteration (train_single_peak_vonMises_KL.py:80), folded in. */
int pnpp_adam_step_dev(float *param, float *grad, float *exp_avg, float *exp_avg_sq, size_t n, uint64_t *step_state,
                       float lr, float beta1, float beta2, float eps, float grad_scale, int zero_grad, void *stream);
/* torch.nn.utils.clip_grad_norm_(parameters, max_norm) (train_multi_peaks_vonMises_KL.py:235) folded into the update with
 * no host round trip: grad_sumsq[0] (device memory, written by pnpp_sumsq on the same stream) is the sum of squares of the
 * flat gradient buffer as it stands; the gradient is grad * grad_scale, its norm sqrt(grad_sumsq[0]) * grad_scale, and the
 * update uses grad * grad_scale * min(1, max_norm / (norm + 1e-6)).  zero_grad != 0 clears each gradient once consumed. */
int pnpp_adam_step_clip(float *param, float *grad, float *exp_avg, float *exp_avg_sq, size_t n, int step, float lr,
                        float beta1, float beta2, float eps, float grad_scale, const double *grad_sumsq, float max_norm,
                        int zero_grad, void *stream);
int pnpp_adam_step_dev_clip(float *param, float *grad, float *exp_avg, float *exp_avg_sq, size_t n, uint64_t *step_state,
                            float lr, float beta1, float beta2, float eps, float grad_scale, const double *grad_sumsq,
                            float max_norm, int zero_grad, void *stream);
/* sum of squares of a flat buffer into out[0] (double), deterministic two-level reduction. */
int pnpp_sumsq(const float *x, size_t n, double *out, void *scratch, size_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * The scheduled optimiser (csrc/optim_sched_kernels.hip, csrc/lr_schedule.h): the update above with parameter groups,
 * weight decay, a learning-rate schedule evaluated on the device and an exponential moving average of the weights, still
 * one launch.  The step count lives in device memory, so a captured launch applies its own rate at every replay.
 * ---------------------------------------------------------------------------------------- */
#define PNPP_OPTIM_MAX_GROUPS 8
enum { PNPP_SCHED_CONSTANT = 0, PNPP_SCHED_COSINE = 1, PNPP_SCHED_STEP = 2 };
typedef struct {
    int n_groups;                                   /* 1 .. PNPP_OPTIM_MAX_GROUPS */
    int decoupled;                                  /* 1: AdamW, p *= 1 - lr_g wd_g; 0: L2 as torch.optim.Adam, g += wd_g p */
    uint64_t end[PNPP_OPTIM_MAX_GROUPS];            /* exclusive end of each group in the flat buffers: strictly increasing,
                                                       end[n_groups - 1] == n.  An element's group is the number of ends <= its index */
    float lr_mult[PNPP_OPTIM_MAX_GROUPS], weight_decay[PNPP_OPTIM_MAX_GROUPS];
    int sched_kind;                                 /* PNPP_SCHED_*: what follows the (optional) linear warm-up */
    uint64_t warmup, total, every;                  /* updates of warm-up; cosine: where it ends; step: updates per decay */
    double start_factor, min_factor, gamma;         /* warm-up starts at start_factor; cosine ends at / step is floored at min_factor */
    float lr, beta1, beta2, eps, grad_scale;
    float max_norm;                                 /* 0: no clipping; else grad_sumsq (pnpp_sumsq's word) is read as in pnpp_adam_step_clip */
    float ema_decay;                                /* 0: no average; else ema = ema_decay ema + (1 - ema_decay) param after the update */
    int zero_grad;                                  /* != 0: clear each gradient once consumed */
} pnpp_optim_desc;
/* One update.  step_state: four words in device memory -- [0] updates taken so far and [1] the ticket, exactly pnpp_adam_step_dev's two
 * (the two entries may alternate on one state); [2] receives the bits of the float64 rate lr * f the update used (f: the schedule's
 * factor at step_state[0], see pnpp_lr_factor); [3] is reserved and left alone.  With lr_g = lr f lr_mult[g] an element of group g sees
 * Adam's update with step size lr_g / (1 - beta1^t), after p *= 1 - lr_g weight_decay[g] (decoupled) or with weight_decay[g] p added to
 * its scaled, clipped gradient (L2).  With one group, lr_mult 1, weight_decay 0, a constant schedule without warm-up and no average the
 * results equal pnpp_adam_step_dev's (pnpp_adam_step_dev_clip's) bit for bit.  ema is null exactly when ema_decay is 0. */
int pnpp_adamw_step(const pnpp_optim_desc *d, float *param, float *grad, float *exp_avg, float *exp_avg_sq, float *ema, size_t n,
                    uint64_t *step_state, const double *grad_sumsq, void *stream);
/* The schedule's factor after steps_taken updates, by the function the kernel evaluates: host arithmetic only, needs no GPU.  Only the
 * schedule fields of the descriptor are read (sched_kind .. gamma). */
int pnpp_lr_factor(const pnpp_optim_desc *d, uint64_t steps_taken, double *factor);

/* ------------------------------------------------------------------------------------------
 * Training-time augmentation of a device-resident batch: a fresh yaw about +Y per cloud (optionally a scale and a
 * clipped Gaussian jitter per point) with the orientation targets moved along, in one launch.
 * The reference rotates its training sets offline (data_process/rotate_without_normals.py:5-15,112 and the GT writers);
 * the conventions are those restated in synthetic.py.
 * ---------------------------------------------------------------------------------------- */
#define PNPP_AUG_MAX_TARGETS 4
#define PNPP_AUG_YAW 1u    /* flags */
#define PNPP_AUG_SCALE 2u
#define PNPP_AUG_JITTER 4u
typedef enum {
    PNPP_AUG_ANGLE = 0, /* (B, rows) angles, cols = 1: mu' = wrap(mu - theta) into (-pi, pi]                              */
    PNPP_AUG_VM = 1,    /* (B, rows, cols) rows [mu, kappa] or [mu, kappa, weight], cols 2 or 3: column 0 as ANGLE, rest copied */
    PNPP_AUG_AXIS = 2,  /* (B, rows, 3) vectors: f' = R f in the points' float32 arithmetic                               */
    PNPP_AUG_DIR8 = 3   /* in (B, 3) forward axis, out (B, 8): relu(dirs8 . R f) / sum, 0.125 each for a zero sum         */
} pnpp_augment_kind;
typedef struct {
    int kind, rows, cols;
    const float *in;
    float *out;
    const int32_t *counts; /* optional (B): only the first counts[b] rows of cloud b are transformed, the rest copied     */
} pnpp_augment_target;
typedef struct {
    unsigned flags;            /* PNPP_AUG_YAW | PNPP_AUG_SCALE | PNPP_AUG_JITTER                                          */
    float scale_lo, scale_hi;  /* SCALE: 0 < lo <= hi, scale = lo + (hi - lo) w1 / 2^32                                     */
    float sigma, clip;         /* JITTER: j = clamp(sigma z, -clip, clip), z standard normal (Box-Muller), both >= 0        */
    int n_targets;             /* <= PNPP_AUG_MAX_TARGETS                                                                   */
    pnpp_augment_target targets[PNPP_AUG_MAX_TARGETS];
    const float *dirs8;        /* (8, 3) unit directions of the DIR8 targets (models/pointnet_pp_8dir.py: DIRS_8)           */
} pnpp_augment_desc;
/* xyz_in (B,N,C) -> xyz_out (B,N,C), out of place, C = 3 (xyz) or 6 (xyz + normal: rotated only).  Rows:
 *   x' = fl(fl(c x) + fl(s z)), y' = y, z' = fl(fl(c z) - fl(s x)), then * scale, then + jitter -- IEEE float32 in this order.
 * Random words are Philox4x32-10 with key (seed) and counter (n, b, stream_id): n = 0xFFFFFFFF gives the cloud's words
 * (w0: theta = w0 2 pi / 2^32, w1: scale), n = point index the point's four (two Box-Muller pairs -> three jitter values);
 * theta, c = cos, s = sin, scale and the jitter are evaluated in float64 and rounded to float32 once.  Without a switch its
 * step is skipped, so with no flag set the output is a copy.  lengths (B) or NULL: rows n >= lengths[b] are copied bit for bit
 * (lengths[b] = 0: the whole cloud; its targets are still transformed).  params_out (B,4) receives [c, s, scale, (float)theta].
 * A pure function of (seed, stream_id, b, n).  B <= 65535, N < 2^32 - 1. */
int pnpp_augment_clouds(uint64_t seed, uint64_t stream_id, const float *xyz_in, float *xyz_out, const int32_t *lengths, int B,
                        int64_t N, int C, const pnpp_augment_desc *desc, float *params_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Surface normals of xyz-only clouds (additive to ABI 5): the neighbour search of pnpp_knn with every point of the cloud as a query,
 * and in the same launch the covariance of each neighbourhood and its smallest eigenvector.  For cloud b, point i:
 *   neighbours    row i of pnpp_knn(xyz, xyz, k): the k smallest (distance, index) keys, the point itself included;
 *   covariance    float64: d_j = (double)p_j - (double)p_i, m = (1/k) sum d_j, C = (1/k) sum d_j d_j^T - m m^T;
 *   normal n      a unit eigenvector of C's smallest eigenvalue l0 (l0 <= l1 <= l2; cyclic Jacobi in float64), its component of
 *                 largest magnitude positive (the lowest index among equal magnitudes), then oriented by s = n . (p_i - ref[b]):
 *                 PNPP_NORMALS_AWAY flips n when s < 0, PNPP_NORMALS_TOWARD when s > 0; s == 0 or PNPP_NORMALS_NONE keep it;
 *   curvature     max(l0, 0) / (l0 + l1 + l2), the surface variation; trace <= 0 (the k neighbours coincide): n = 0, curvature 0.
 * Each is rounded to float32 once.  Where l0 and l1 nearly coincide n is some unit vector of that eigenspace.
 * out (B,N,out_stride): out_stride 3 holds n; out_stride 6 holds the point in columns 0-2 and n in 3-5 (what pnpp_augment_clouds
 * takes at C = 6).  curv (B,N) and idx (B,N,k) are optional.  ref (B,3) float32 is required by the two orienting modes.
 * 3 <= k <= 128 and k <= N (PNPP_ERR_RANGE, as pnpp_knn); B <= 65535.  No atomics: two calls give the same bits.
 * _ragged: lengths (B) int32 on the device as for pnpp_knn_ragged -- row b is the call on xyz[b, :lengths[b]] alone, bit for bit; the
 * input rows at or beyond lengths[b] are never read and their rows of out, curv and idx are zeros. */
#define PNPP_NORMALS_NONE 0
#define PNPP_NORMALS_AWAY 1
#define PNPP_NORMALS_TOWARD 2
int pnpp_estimate_normals(const float *xyz, int B, int N, int k, int orient, const float *ref, float *out, int out_stride, float *curv,
                          int32_t *idx, void *stream);
int pnpp_estimate_normals_ragged(const float *xyz, int B, int N, const int32_t *lengths, int k, int orient, const float *ref, float *out,
                                 int out_stride, float *curv, int32_t *idx, void *stream);

/* ------------------------------------------------------------------------------------------
 * Yaw symmetry of a cloud from its own geometry (additive to ABI 5): under which rotations about +Y does the cloud map onto itself?
 * For cloud b with valid points p_i (i < Nv), centre c = centre[b] (x and z are used) and table rows (cs_g, sn_g), g < G -- every
 * float32 step one IEEE operation, in this order, unfused:
 *   centre       q_i = (p_i.x - c.x, p_i.y, p_i.z - c.z);
 *   rotate       x' = fl(fl(cs x) + fl(sn z)), z' = fl(fl(cs z) - fl(sn x)), y' = y       (pnpp_augment_clouds' order);
 *   nearest      d[g,i] = min over j < Nv of (dx dx + dy dy) + dz dz between rot_g(q_i) and q_j, the lowest j among equal distances;
 *   profile      D[b,g] = (float) (sum_i (double) d[g,i] / Nv), the sum in float64 in a fixed order;
 *   floor        nu[b]: the same at the identity rotation (1, 0) with j != i -- the mean squared distance to the nearest OTHER point;
 *                0 when Nv = 1.
 * pnpp_yaw_profile leaves per-workgroup float64 partial sums in `workspace` (pnpp_yaw_workspace_bytes(B, N, G) bytes, 0 with a message
 * for non-positive sizes); nearest_dist / nearest_idx (B,G,N), both or neither, receive d[g,i] and its j (0 and -1 for i >= Nv).
 * _ragged: lengths (B) int32 on the device, Nv = min(max(lengths[b], 1), N); rows at or beyond Nv are never read (they may hold NaN).
 * pnpp_yaw_symmetry finishes the sums of that workspace (same B, N, lengths, G) into distance (B,G) and floor (B) and, when the four
 * decision outputs are given (all or none), forms
 *   S[g] = D[g] + D[(G - g) % G]      the symmetric Chamfer distance: the mirror index is the other direction;
 *   score[g] = S[g] / (2 nu)          reported only (inf or nan where nu = 0);
 *   bound = fl(fl(2 nu) tol);         order 0 (continuous) if S[g] <= bound for every g >= 1; else the largest m of `orders` with
 *                                     S[k G / m] <= bound for k = 1..m-1; else 1.  The table is taken to be the uniform grid 2 pi g / G.
 * count (B) = order; angles (B, angle_stride) = (float) (2 pi k / order) for k < order, zeros beyond.  `orders` is a HOST array of
 * n_orders <= PNPP_YAW_MAX_ORDERS values, each >= 2 and dividing G; angle_stride >= the largest of them; tol finite and >= 0.
 * No atomics: two calls give the same bits.  Both launches can be captured in a graph; nothing is read back.  B <= 65535. */
#define PNPP_YAW_ANGLE_BLOCK 8   /* rotations a lane holds for its query (one of them the floor, in a cloud's first block)     */
#define PNPP_YAW_TILE 1024       /* candidates staged in LDS per pass: N above it loops                                       */
#define PNPP_YAW_QUERIES 256     /* queries per workgroup                                                                     */
#define PNPP_YAW_MAX_ORDERS 16
size_t pnpp_yaw_workspace_bytes(int B, int N, int G);
int pnpp_yaw_profile(const float *xyz, int B, int N, const float *centre, const float *table, int G, void *workspace,
                     size_t workspace_bytes, float *nearest_dist, int32_t *nearest_idx, void *stream);
int pnpp_yaw_profile_ragged(const float *xyz, int B, int N, const int32_t *lengths, const float *centre, const float *table, int G,
                            void *workspace, size_t workspace_bytes, float *nearest_dist, int32_t *nearest_idx, void *stream);
int pnpp_yaw_symmetry(const void *workspace, size_t workspace_bytes, int B, int N, const int32_t *lengths, int G, float tol,
                      const int32_t *orders, int n_orders, float *distance, float *floor, float *score, int32_t *order, int32_t *count,
                      float *angles, int angle_stride, void *stream);

/* ------------------------------------------------------------------------------------------
 * Single-view scan simulation (additive to ABI 5): what one viewer at infinity sees of each cloud -- an orthographic depth-buffer
 * visibility test, survivors compacted in input order.  For cloud b with valid rows n < Nv (Nv = min(max(lengths_in[b], 1), N), or N
 * when lengths_in is NULL); every float32 step one IEEE operation, in this order, unfused:
 *   direction    Philox4x32-10 words w of counter (0xFFFFFFFF, b, stream_id), key seed (pnpp_augment_clouds' cloud words):
 *                azimuth phi = w0 2 pi / 2^32 about +Y, elevation eps = lo + (hi - lo) w1 / 2^32; ca, sa, ce, se = cos / sin of the
 *                two in float64, each rounded to float32 once; v = (ce sa, se, -ce ca) towards the viewer, r = (ca, 0, sa),
 *                u = (-se sa, ce, se ca).  PNPP_VIEW_ANGLES: view_dirs (B,2) holds [phi, eps] and nothing is drawn; PNPP_VIEW_DIRS:
 *                view_dirs (B,3) holds a direction towards the viewer, normalised in float64 to (nx, ny, nz): se = ny,
 *                ce = sqrt(nx^2 + nz^2), sa = nx / ce, ca = -nz / ce (ce = 0, straight up or down: sa = 0, ca = 1; a zero or
 *                non-finite direction: phi = eps = 0), and phi = atan2(sa, ca), eps = atan2(se, ce) are reported;
 *   projection   d = p . v, a = p . r, t = p . u, each fl(fl(fl(x e_x) + fl(y e_y)) + fl(z e_z));
 *   extent       amin, amax, tmin, tmax over the valid rows (a zero taken as +0), ext = max(amax - amin, tmax - tmin), cell = ext / G,
 *                ia = min(G - 1, floor((a - amin) / cell)), it likewise from t and tmin; both 0 unless cell > 0;
 *   depth buffer zmax[i, j] = the largest d among the points whose own cell lies within `splat` cells of (i, j) in both directions;
 *   test         a point is visible iff fl(zmax[ia, it] - d) <= fl(thickness ext);
 *   thinning     drop > 0: the cloud's ratio is drop w2 / 2^32, and a visible point survives iff word 0 of its own Philox words
 *                (counter (n, b, stream_id)) is >= fl64(drop w2) -- the ratio times 2^32;
 *   compaction   survivors keep their order: rows 0 .. kept-1 of xyz_out (C = 6: the normal travels untouched), rows kept .. N-1 exact
 *                zeros; lengths_out[b] = kept; index_out (B,N), optional: the source row of each output row, -1 in the padding;
 *   floor        kept < min_keep: the cloud passes through whole -- its Nv rows, lengths_out[b] = Nv, index n.
 * params_out (B,8) = [v_x, v_y, v_z, (float) phi, (float) eps, cell, kept, passed_through (1 or 0)].  Rows at or beyond Nv are never
 * read (they may hold NaN).  One launch, one workgroup per cloud, no global atomics, nothing read back: two calls give the same bits and
 * the call can be captured in a graph.  A pure function of (seed, stream_id, b, n).
 * PNPP_ERR_ARG: a null xyz_in, xyz_out, lengths_out, desc or params_out; xyz_in == xyz_out; C not 3 or 6; B outside 1..65535; N outside
 * 1..2^24; G outside 1..PNPP_VIEW_MAX_G; splat outside 0..2; thickness negative or not finite; an elevation range outside
 * [-pi/2, pi/2] (as float32) or reversed; drop outside [0, 1); min_keep outside 0..N; unknown flag bits, both view flags, or view_dirs
 * without its flag. */
#define PNPP_VIEW_MAX_G 128
#define PNPP_VIEW_DIRS 1u   /* flags: view_dirs is (B,3), directions towards the viewer */
#define PNPP_VIEW_ANGLES 2u /*        view_dirs is (B,2), [azimuth, elevation] in radians */
typedef struct {
    int G;                  /* cells a side of the depth buffer, 1..PNPP_VIEW_MAX_G                                          */
    int splat;              /* a point covers the (2 splat + 1)^2 cells around its own, 0..2                                  */
    float thickness;        /* visible within this fraction of the extent behind the front surface, >= 0                     */
    float elev_lo, elev_hi; /* the drawn elevation's range, -pi/2 <= lo <= hi <= pi/2                                        */
    float drop;             /* thinning of the visible points, [0, 1): the cloud's ratio is uniform in [0, drop)             */
    int min_keep;           /* fewer survivors than this: the cloud passes through whole, 0..N                               */
    unsigned flags;         /* PNPP_VIEW_DIRS or PNPP_VIEW_ANGLES, or 0: the direction is drawn                              */
    const float *view_dirs; /* device pointer, or NULL with flags 0                                                          */
} pnpp_view_desc;
int pnpp_view_clouds(uint64_t seed, uint64_t stream_id, const float *xyz_in, float *xyz_out, const int32_t *lengths_in,
                     int32_t *lengths_out, int32_t *index_out, int B, int64_t N, int C, const pnpp_view_desc *desc, float *params_out,
                     void *stream);

/* ------------------------------------------------------------------------------------------
 * Raw-scan preparation (additive to ABI 5): voxel-grid downsample, statistical outlier removal, unit frame.  Each entry has
 * pnpp_view_clouds' contract: rows (B,N,C) float32 with C 3 or 6 (columns 3..5 travel unchanged), cloud b's valid rows n < Nv
 * (Nv = min(max(lengths_in[b], 1), N), or N when lengths_in is NULL) must be finite, rows at or beyond Nv are never read (they may hold
 * NaN); survivors keep their order in rows 0 .. kept-1 of xyz_out, rows kept .. N-1 are exact zeros, lengths_out[b] = kept,
 * index_out (B,N), optional: the source row of each output row, -1 in the padding.  Out of place; nothing is read back, no
 * floating-point atomics: two calls give the same bits and the calls can be captured in a graph.  Every float32 step below is one IEEE
 * operation, in this order, unfused (tests/scan_ref.py restates them).
 *
 * pnpp_voxel_downsample: one real point per occupied cell -- the one nearest the cell's centre (Open3D and PCL return the cell's
 * centroid instead: an averaged point has no source row, its normal means nothing, and its bits depend on a summation order).
 *   bounds   lo[a], hi[a]: min and max over the valid rows per axis, a zero of either sign taken as +0;
 *   edge     h = cell, or with grid > 0  h = max_a(hi[a] - lo[a]) / (float) grid; h = 1 unless h > 0;
 *   cell     c[a] = min(max(floor((x[a] - lo[a]) / h), 0), last), last = 1023: ten bits per axis, cells beyond index 1023 merge
 *            into the last; with grid, last = grid - 1: the far face of the longest axis belongs to the last cell (grid = 1: one cell);
 *   centre   m[a] = lo[a] + (c[a] + 0.5) h;  d = (x0 - m0)^2 + (x1 - m1)^2 + (x2 - m2)^2, summed in that order;
 *   winner   per cell the row with the smallest 64-bit key (bits(d) << 32) | n: nearest the centre, lowest row among equals.
 * Exactly one of cell (finite, > 0; grid = 0) and grid (1..PNPP_VOXEL_MAX_GRID; cell = 0).  workspace: pnpp_voxel_workspace_bytes(B, N)
 * bytes (0: B or N refused), the per-cloud open-addressing table (at least 2 N slots) and the bounds; the call clears it itself.  Four
 * launches: clear, bounds, insert (several workgroups per cloud; compare-and-swap claims a cell's slot, an unsigned 64-bit atomicMin
 * takes the winner), compact (one workgroup per cloud).
 *
 * pnpp_outlier_statistic: lists (B,N,k+1) int32 neighbour rows of every point (pnpp_knn_ragged of the cloud on itself with k + 1);
 * statistic[b, n] = (sum_j sqrt((double) d(x_n, x_list[j]))) / k in float64 in list order over all k + 1 entries (the point itself adds
 * 0, listed or not), 0 for n >= Nv.  pnpp_outlier_filter: mean and population standard deviation of the statistic over the valid rows
 * in float64 in a fixed order, thr = mean + std_ratio std, a row is kept iff statistic <= thr; a cloud with Nv <= k passes through
 * whole.  stats_out (B,4) float64, optional: [mean, std, thr, kept] ([0, 0, inf, Nv] for a cloud that passed through).
 * 1 <= k <= PNPP_OUTLIER_MAX_K; std_ratio finite and >= 0.
 *
 * pnpp_normalize_clouds: x' = (x - centre) / scale, one launch, one workgroup per cloud.  centre: PNPP_SCAN_NONE (0), PNPP_SCAN_CENTROID
 * (the float64 mean of the valid rows, fixed order, rounded to float32) or PNPP_SCAN_BOX (0.5 (lo + hi)); scale: PNPP_SCAN_NONE (1),
 * PNPP_SCAN_SPHERE (sqrt(max_n |x_n - centre|^2), the squares summed x, y, z) or PNPP_SCAN_BOX (0.5 max_a(hi[a] - lo[a])); 1 unless > 0.
 * centre_out (B,3) and scale_out (B) map a result back.  Rows at or beyond Nv come back as zeros.
 *
 * PNPP_ERR_ARG: a null pointer other than lengths_in, index_out, stats_out; xyz_in == xyz_out; C not 3 or 6; B outside 1..65535;
 * N outside 1..2^24; cell and grid both or neither, grid above PNPP_VOXEL_MAX_GRID; a workspace too small; k or std_ratio out of range;
 * an unknown mode. */
#define PNPP_VOXEL_MAX_GRID 1024
#define PNPP_OUTLIER_MAX_K 127 /* the search lists k + 1 <= 128 rows */
#define PNPP_SCAN_NONE 0
#define PNPP_SCAN_CENTROID 1 /* centre */
#define PNPP_SCAN_SPHERE 1   /* scale  */
#define PNPP_SCAN_BOX 2      /* either */
size_t pnpp_voxel_workspace_bytes(int B, int64_t N);
int pnpp_voxel_downsample(const float *xyz_in, float *xyz_out, const int32_t *lengths_in, int32_t *lengths_out, int32_t *index_out, int B,
                          int64_t N, int C, float cell, int grid, void *workspace, size_t workspace_bytes, void *stream);
int pnpp_outlier_statistic(const float *xyz, const int32_t *lists, const int32_t *lengths, int B, int64_t N, int C, int k,
                           double *statistic, void *stream);
int pnpp_outlier_filter(const float *xyz_in, float *xyz_out, const double *statistic, const int32_t *lengths_in, int32_t *lengths_out,
                        int32_t *index_out, double *stats_out, int B, int64_t N, int C, int k, double std_ratio, void *stream);
int pnpp_normalize_clouds(const float *xyz_in, float *xyz_out, const int32_t *lengths, int B, int64_t N, int C, int centre_mode,
                          int scale_mode, float *centre_out, float *scale_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PNPP_HIP_H */
