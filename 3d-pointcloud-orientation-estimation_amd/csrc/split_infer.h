// split_infer.h -- device routine shared by the forward-only kernels (sa_infer_kernels.hip, pointnet_infer_kernels.hip,
// transformer_infer_kernels.hip): the split-product tile loop over fragment-major weight planes.  The exact three-way split of float32
// into bfloat16 pieces that feeds it is in split_prims.h.
#pragma once
#include "split_prims.h"

namespace pnpp {
namespace {

// acc[j] + accl[j] += act[32 rows][0 .. Kd) * W[col_j .. +32][0 .. Kd)^T for NJ column blocks `colstep` apart, float32 products formed
// on v_mfma_f32_32x32x16_bf16 from the three-way splits of both operands: a b = a_h b_h + (a_l b_h + a_h b_l + a_m b_m + a_m b_h +
// a_h b_m) + [below 2^-25 |a b|, dropped]; every product kept is exact in float32.  The leading products accumulate in acc, the five
// small ones in accl (the instruction aligns its addends to the largest exponent and drops what lies 2^-26 below: small addends must
// not meet the large sum inside it); the caller adds the two once.  Six instructions of 32 cycles per 16 reduction steps against
// eight of 64 on v_mfma_f32_32x32x2_f32.  Lane l = 32 h + r holds A[row r][k = 8 h + j] and B[k = 8 h + j][column r], j = 0 .. 7.
template <int NJ>
__device__ __forceinline__ void infer_chunk(const unsigned short *__restrict__ act, int ld, size_t aplane, int Kd,
                                            const unsigned short *__restrict__ W, size_t wplane, int col0, int colstep, f32x16 (&acc)[NJ],
                                            f32x16 (&accl)[NJ]) {
    const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
    const unsigned short *ap = act + (size_t)r * ld + 8 * h;
    const unsigned short *bp[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bp[j] = W + (size_t)((col0 + j * colstep) >> 5) * (Kd >> 4) * 512 + (threadIdx.x & 63) * 8;
    uint4 a[3], bv[NJ][3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        a[p] = *reinterpret_cast<const uint4 *>(ap + p * aplane);
#pragma unroll
        for (int j = 0; j < NJ; ++j) bv[j][p] = *reinterpret_cast<const uint4 *>(bp[j] + p * wplane);
    }
    for (int k0 = 0; k0 < Kd; k0 += 16) {
        uint4 an[3], bn[NJ][3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            an[p] = a[p];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bn[j][p] = bv[j][p];
        }
        if (k0 + 16 < Kd) {   // the next step's fragments are in flight while this one is multiplied
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                an[p] = *reinterpret_cast<const uint4 *>(ap + p * aplane + k0 + 16);
#pragma unroll
                for (int j = 0; j < NJ; ++j) bn[j][p] = *reinterpret_cast<const uint4 *>(bp[j] + p * wplane + (size_t)(k0 + 16) * 32);
            }
        }
        const bf16x8 ah = __builtin_bit_cast(bf16x8, a[0]), am = __builtin_bit_cast(bf16x8, a[1]), al = __builtin_bit_cast(bf16x8, a[2]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const bf16x8 bh = __builtin_bit_cast(bf16x8, bv[j][0]), bm = __builtin_bit_cast(bf16x8, bv[j][1]),
                         bl = __builtin_bit_cast(bf16x8, bv[j][2]);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[j], 0, 0, 0);
            accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, accl[j], 0, 0, 0);
            accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, accl[j], 0, 0, 0);
            accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, accl[j], 0, 0, 0);
            accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, accl[j], 0, 0, 0);
            accl[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, accl[j], 0, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            a[p] = an[p];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bv[j][p] = bn[j][p];
        }
    }
}

}  // namespace
}  // namespace pnpp
