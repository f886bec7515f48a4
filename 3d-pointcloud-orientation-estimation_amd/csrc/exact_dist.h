// exact_dist.h -- the exact float32 distance recipes of the index kernels (knn_kernels.hip, sampling_kernels.hip, group_kernels.hip).
//
// Bit-exactness: the float32 arithmetic below reproduces the evaluation order of the reference's CPU PyTorch path (SURVEY.md 8a-2;
// oracle/index_ops.c is the CPU restatement), with explicit fmaf where -- and only where -- ATen fuses.  Every file that includes this
// header is compiled with -ffp-contract=off (pnpp_hip/build.py: SOURCES) and carries `#pragma clang fp contract(off)` ahead of the
// include, so the compiler introduces no fused multiply-add of its own here or in the kernels that call these.
#pragma once
#include "common.h"

namespace pnpp {

// models/base.py:25-26  torch.sum(p**2, -1): (x^2 + y^2) + z^2, unfused
__device__ __forceinline__ float sq3_exact(float x, float y, float z) {
    float s = __fmul_rn(x, x);
    s = __fadd_rn(s, __fmul_rn(y, y));
    s = __fadd_rn(s, __fmul_rn(z, z));
    return s;
}
// models/base.py:24-26  -2*matmul (K=3 sgemm: fma chain) then += |a|^2 then += |b|^2
__device__ __forceinline__ float pair_dist_exact(float ax, float ay, float az, float bx, float by, float bz, float sa,
                                                 float sb) {
    float dot = __fmaf_rn(az, bz, __fmaf_rn(ay, by, __fmul_rn(ax, bx)));
    float d = __fmul_rn(-2.0f, dot);
    d = __fadd_rn(d, sa);
    d = __fadd_rn(d, sb);
    return d;
}
// PointNet++Demo.py:25,63  torch.sum((a-b)**2, -1): direct form, unfused
__device__ __forceinline__ float direct_dist_exact(float ax, float ay, float az, float bx, float by, float bz) {
    float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    float d = __fmul_rn(dx, dx);
    d = __fadd_rn(d, __fmul_rn(dy, dy));
    d = __fadd_rn(d, __fmul_rn(dz, dz));
    return d;
}

}  // namespace pnpp
