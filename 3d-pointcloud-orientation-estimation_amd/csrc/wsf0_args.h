// wsf0_args.h -- what gemm_wsf0_kernel (gemm_wsx_kernels.hip) and its split-product form gemm_wsf03_kernel (gemm_wsf03_kernels.hip) share:
// the argument block and the moment-partial layout.
#pragma once
#include "kernels.h"

namespace pnpp {

constexpr int kMomSlabs = 128, kMomPitch = 16;

struct Wsf0Args {
    const float *xyz, *centres;
    const int32_t *idx;
    int M, N, S;
    const float *W0;   // 64 x 3, pitch ldw0
    int ldw0;
    // layer 0's BatchNorm: train mode finishes the statistics from the moment partials (mom, nmom); eval mode reads scale0 / shift0
    const double *mom;
    int nmom, training;
    const float *bias0, *gamma0, *beta0;
    float *rm0, *rv0;
    long long *nbt0;
    float momentum, eps;
    float *mean0, *istd0, *scale0, *shift0;
    const float *W1;   // C_1 x 64 as stored (row = output channel)
    int ldw1;
    float *z1;         // M x 64
    double *slab;      // [workers][2][64] (EM == E_STORE_STATS)
    int store_policy;  // StorePolicy bits (common.h); gemm_wsf03_kernel honours them
};

// the split-product form (float32 products from exact three-way bf16 splits; on with split_products() unless PNPP_WSF03=0)
bool wsf03_enabled();
void launch_wsf03(const Wsf0Args &P, int workers, int epilogue_mode, hipStream_t st);

}  // namespace pnpp
