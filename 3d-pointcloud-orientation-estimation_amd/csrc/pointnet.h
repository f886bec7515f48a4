// pointnet.h -- launchers of the vanilla PointNet kernels (csrc/pointnet_kernels.hip), called by csrc/pointnet_api.hip.
#pragma once
#include "common.h"

namespace pnpp {

// Ragged batches: every launcher that addresses point rows per cloud takes `offs`, the device int32 array of B + 1 exclusive prefix
// sums of the clouds' lengths (row n of cloud b at offs[b] + n), or nullptr for a uniform batch (row b * N + n).  M is the number of
// point rows the BatchNorm statistics run over: B * N, or the sum of the lengths.  Grids are sized by the padded N either way.

// lengths (B) on the device -> their clamp into 1 .. N and the B + 1 offsets
int launch_pn_offsets(const int32_t *lengths, int B, int N, int32_t *lens_out, int32_t *offs, hipStream_t st);

// ---- pooled wide layer: max_n act(BN(A_n W^T + b)) per cloud, nothing of size (B*N) x C stored ----
// forward, train mode: per-cloud column sums and Gram matrix of A (float64), their sums over the clouds and the centred Gram
// matrix Cc = G - S S^T / M
int pn_gram_slices(int N);   // row slices per cloud of the Gram launch (its partials: B * slices)
int launch_pn_gram(const float *a, const int32_t *offs, long long M, int B, int N, int K, double *gp, double *sp, double *S, double *Cc,
                   hipStream_t st);
// forward: the cloud's max / min of z = A W^T + b per channel and their (first) rows
int launch_pn_pool_scan(const float *a, const int32_t *offs, const float *w, const float *bias, int B, int N, int K, int C, float *zmax,
                        int32_t *imax, float *zmin, int32_t *imin, hipStream_t st);
// forward: statistics (train: from S / Cc; eval: running), pooled output, routes, running statistics
int launch_pn_pool_finalize(const float *w, const float *bias, const float *gamma, const float *beta, const double *S, const double *Cc,
                            const float *zmax, const int32_t *imax, const float *zmin, const int32_t *imin, int B, long long M, int K, int C,
                            int relu, int training, float eps, float momentum, float *rm, float *rv, long long *nbt, float *mean,
                            float *istd, float *zsel, float *ypre, int32_t *route, float *out, hipStream_t st);
// backward, per channel: dgamma, dbeta, db, dW, the routed coefficients a_c h_{b,c} and the vectors u = a g, v = a m istd
int launch_pn_pool_bwd_channels(const float *a, const int32_t *offs, long long M, const float *w, const float *gamma, const float *dout, const float *mean,
                                const float *istd, const float *zsel, const float *ypre, const int32_t *route, const double *S,
                                const double *Cc, int B, int N, int K, int C, int relu, int training, float *dw, float *db,
                                float *dgamma, float *dbeta, float *coef, float *u, float *v, hipStream_t st);
// backward, train mode: Q = W^T diag(v) W and cvec = -W^T u
int launch_pn_pool_bwd_q(const float *w, const float *u, const float *v, int K, int C, float *Q, float *cvec, hipStream_t st);
// backward: dA_n = R_n + cvec - Q (A_n - S/M) (train) or R_n (eval), R the routed scatter of coef_{b,c} w_c
int launch_pn_pool_bwd_da(const float *a, const int32_t *offs, long long M, const float *w, const float *Q, const float *cvec, const float *coef, const int32_t *route,
                          const double *S, int B, int N, int K, int C, int training, float *da, hipStream_t st);

// ---- per-cloud transform Y_b = X_b T_b (first k columns), columns k..D-1 passed through, columns D..ldy-1 zero ----
// with offs: y / dy are packed rows; x / dx padded (dx zero at padding rows), or packed rows of pitch sn themselves when xpacked
int launch_pn_transform(const float *x, const int32_t *offs, int xpacked, long long sb, long long sn, long long sd, const float *t, int B,
                        int N, int D, int k, int ldy, float *y, hipStream_t st);
int launch_pn_transform_bwd(const float *x, const int32_t *offs, int xpacked, long long sb, long long sn, long long sd, const float *t,
                            const float *dy, int B, int N, int D, int k, int ldy, float *dx, float *dt, hipStream_t st);

// ---- feature-transform regulariser mean_b ||T_b T_b^T - I||_F ----
int launch_pn_regularizer(const float *t, int B, int k, double *norms, float *out, hipStream_t st);
int launch_pn_regularizer_bwd(const float *t, const double *norms, const float *dout, int B, int k, float *dt, hipStream_t st);

// ---- small pieces of the heads / encoder output ----
int launch_pn_add_identity(const float *x, int B, int k, float *y, hipStream_t st);
// with offs: pf / dpf are packed rows (pf_padded: pf has B * N rows all the same), out is zero and dout unread at padding columns
int launch_pn_concat(const float *g, const float *pf, const int32_t *offs, int pf_padded, int B, int N, int C1, int C2, float *out,
                     hipStream_t st);
int launch_pn_concat_bwd(const float *dout, const int32_t *offs, int B, int N, int C1, int C2, float *dg, float *dpf, hipStream_t st);
int launch_pn_bn_relu(const float *x, int M, int C, const float *gamma, const float *beta, float *rm, float *rv, long long *nbt,
                      int training, float eps, float momentum, float *mean, float *istd, float *y, hipStream_t st);
int launch_pn_bn_relu_bwd(const float *x, const float *y, const float *dy, int M, int C, const float *gamma, const float *mean,
                          const float *istd, int training, float *dx, float *dgamma, float *dbeta, hipStream_t st);

}  // namespace pnpp
