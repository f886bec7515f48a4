// fc.h -- launchers of the fully connected block's kernels (csrc/fc_kernels.hip), called by csrc/fc_api.hip.
#pragma once
#include "kernels.h"

namespace pnpp {

constexpr int FC_SMALL_N = 16;   // at most this many outputs and no normalisation: the dot-product kernels (fc_small_*), no MFMA tile

// How a backward kernel rebuilds g = d loss / d (normalised, activated output) from what the forward pass kept: g = dy with the
// dropout mask and the ReLU gate applied; the BatchNorm-backward terms come from scale .. istd (bn != 0) or the gate from the bias
// (bn == 0).  LayerNorm reads mean / istd per ROW and takes its affine parameters beside this.
struct FcGrad {
    const float *dy, *z;
    const uint8_t *mask;
    float drop_scale;
    int relu, bn, training;
    const float *scale, *shift, *mean, *istd, *bias;
    int M, N;
};
// the keep-mask drawn in the kernel (mask_out null: no draw); rng_counter = [stream id, ticket word] in device memory
struct FcDraw {
    uint8_t *mask_out = nullptr;
    float drop_p = 0.f;
    unsigned long long rng_seed = 0;
    unsigned long long *rng_counter = nullptr;
};

inline int fc_row_chunks(int M) { return cdiv(M, 256); }   // the row-chunked backward kernels: one [N] (or [2N]) partial per 256 rows

// ---- forward ----
// y = dropout(relu(z * scale + shift)); scale null: y = dropout(relu(z + shift)).  tagged: whether the launch is recorded under a
// ProfScope (it is not when it follows a BatchNorm finalisation in the forward pass); what: the label of a failed launch
int launch_fc_apply_cols(const float *z, const float *scale, const float *shift, const uint8_t *mask, float drop_scale, int relu, int M,
                         int N, float *y, bool tagged, const char *what, hipStream_t st);
int launch_fc_apply_ln(const float *z, const float *b, const float *nw, const float *nb, const uint8_t *mask, float drop_scale, int relu,
                       int M, int N, float eps, float *y, float *mean, float *istd, const FcDraw &draw, hipStream_t st);
int launch_fc_small_fwd(const float *x, const float *w, const float *b, const uint8_t *mask, float drop_scale, int relu, int M, int K, int N,
                        float *z, float *y, hipStream_t st);

// ---- backward: dz (M x N) and the parameter gradients pg of the normalisation (dbias: the linear bias) ----
// no normalisation, many rows: dz and fc_row_chunks(M) partials [chunk][N] of the bias gradient in slab
int launch_fc_bwd_rows(const FcGrad &g, float *dz, float *slab, hipStream_t st);
// BatchNorm / none, every workgroup all rows of its columns.  phase 0: one pass; SyncBN: phase 1 (sums to glob / local), the
// exchange, phase 2 (apply)
int launch_fc_bwd_cols(const FcGrad &g, float *dz, const BnGrads &pg, int phase, double *glob, double *local, hipStream_t st);
// BatchNorm, many rows: float64 partials [chunk][2N], then the apply pass
int launch_fc_bwd_bn_rows_sums(const FcGrad &g, double *part, hipStream_t st);
int launch_fc_bwd_bn_rows_apply(const FcGrad &g, const double *part, float *dz, const BnGrads &pg, hipStream_t st);
// LayerNorm: rows (dz and the masked gradient gbuf), then the column sums
int launch_fc_bwd_ln_rows(const FcGrad &g, const float *nw, const float *nb, float *dz, float *gbuf, hipStream_t st);
int launch_fc_bwd_ln_cols(const FcGrad &g, const float *gbuf, const float *dz, const BnGrads &pg, hipStream_t st);
// at most 32 rows, BatchNorm / none: dz never written -- dx, dW and pg in one launch; fc_bwd_fused_lds: the dynamic LDS it asks for
size_t fc_bwd_fused_lds(int N);
int launch_fc_bwd_fused(const FcGrad &g, const float *w, const float *x, int K, float *dx, float *dw, const BnGrads &pg, hipStream_t st);
// narrow layer: dW, db and (dx non-null) dx in one launch
int launch_fc_small_bwd(const FcGrad &g, const float *x, const float *w, int K, float *dw, float *db, float *dx, hipStream_t st);
// dW (N x K) = dz^T x for at most 32 rows, written in place
int launch_dw_fewrows(const float *dz, const float *x, int M, int N, int K, float *dw, hipStream_t st);

}  // namespace pnpp
