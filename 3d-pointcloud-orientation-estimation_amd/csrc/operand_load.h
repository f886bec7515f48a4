// operand_load.h -- the device-side A-operand loaders of the fused GEMMs, ONE definition: how a row of the A operand (AOperand, kernels.h)
// is fetched and transformed on its way into a kernel.  Used by the generic and the small-M kernel and dZ materialisation
// (gemm_kernels.hip, gemm_smallm.h) and by the dW kernels (dw_kernels.hip).
//
// Device code only, every function __forceinline__: nothing here is emitted on its own, and there is no host code.
#pragma once
#include "kernels.h"

namespace pnpp {

// ---------------------------------------------------------------------------------------------
// A-operand loaders: four consecutive k of one row, split into a raw fetch (global loads only, so
// the next chunk's loads can be in flight while the current chunk is in the MFMA loop) and a
// transform applied when the chunk is written to LDS.
// ---------------------------------------------------------------------------------------------
struct RawA {
    float4 p, q;  // p: primary values; q: z (A_DZ*) or the centre coordinates to subtract (A_GATHER xyz part)
    int4 ia;      // A_DZ_POOL: arg-max neighbour of the row's group, per channel
};

// Loads are UNCONDITIONAL on clamped (always valid) addresses and masked afterwards: a load inside a
// per-lane branch makes hipcc branch around it and drain vmcnt(0) per element, which serialises the
// whole prefetch (cdna_hip_programming.md, "three .s-level traps", item c).
template <int MODE>
__device__ __forceinline__ RawA fetch_a4(const AOperand &A, int row, int k, int M, int Kd) {
    RawA r;
    r.p = make_float4(0.f, 0.f, 0.f, 0.f);
    r.q = make_float4(0.f, 0.f, 0.f, 0.f);
    r.ia = make_int4(0, 0, 0, 0);
    const int rc = min(row, M - 1);
    if constexpr (MODE == A_PLAIN || MODE == A_BNRELU) {
        const int kc = min(k, Kd - 4);
        r.p = *reinterpret_cast<const float4 *>(A.a + (size_t)rc * A.lda + kc);
    } else if constexpr (MODE == A_DZ) {
        const int kc = min(k, Kd - 4);
        r.p = *reinterpret_cast<const float4 *>(A.a + (size_t)rc * A.lda + kc);
        r.q = *reinterpret_cast<const float4 *>(A.z + (size_t)rc * A.lda + kc);
    } else if constexpr (MODE == A_DZ_POOL) {
        const int kc = min(k, Kd - 4);
        const size_t g = (size_t)(rc / A.K);
        r.p = *reinterpret_cast<const float4 *>(A.a + g * A.lda + kc);
        r.ia = *reinterpret_cast<const int4 *>(A.arg + g * A.lda + kc);
        r.q = *reinterpret_cast<const float4 *>(A.z + (size_t)rc * A.lda + kc);
    } else {  // A_GATHER / A_CONCAT: features first, then xyz (relative to the centre when gathering)
        size_t prow = (size_t)rc, grp = 0;
        if constexpr (MODE == A_GATHER) {
            grp = (size_t)(rc / A.K);  // centre row (b*S + s)
            prow = (size_t)(grp / A.S) * A.N + A.idx[rc];
        }
        if ((A.D & 3) == 0 && A.D >= 4) {
            // whole float4 groups are either features (k < D) or the [x y z 0] tail (k == D)
            const float4 f = *reinterpret_cast<const float4 *>(A.a + prow * A.D + min(k, A.D - 4));
            const float *xp = A.xyz + prow * 3;
            const float x0 = xp[0], x1 = xp[1], x2 = xp[2];
            float c0 = 0.f, c1 = 0.f, c2 = 0.f;
            if constexpr (MODE == A_GATHER) {
                const float *cp = A.new_xyz + grp * 3;
                c0 = cp[0], c1 = cp[1], c2 = cp[2];
            }
            const bool feat = k < A.D;
            r.p = feat ? f : make_float4(x0, x1, x2, 0.f);
            r.q = feat ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(c0, c1, c2, 0.f);
        } else {
            float pv[4], qv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = k + i;
                const bool feat = kk < A.D;
                const int xc = min(max(kk - A.D, 0), 2);
                const float *src = feat ? A.a + prow * A.D + kk : A.xyz + prow * 3 + xc;
                const float v = *src;
                float cv = 0.f;
                if constexpr (MODE == A_GATHER) cv = A.new_xyz[grp * 3 + xc];
                const bool valid = kk < A.D + 3;
                pv[i] = valid ? v : 0.f;
                qv[i] = (valid && !feat) ? cv : 0.f;
            }
            r.p = make_float4(pv[0], pv[1], pv[2], pv[3]);
            r.q = make_float4(qv[0], qv[1], qv[2], qv[3]);
        }
    }
    return r;
}

template <int MODE>
__device__ __forceinline__ void xform_a4(const AOperand &A, const RawA &r, int row, int k, int M, int Kd, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (row >= M || k >= Kd) return;  // padding rows/columns must be exact zeros AFTER the transform
    if constexpr (MODE == A_PLAIN) {
        v[0] = r.p.x, v[1] = r.p.y, v[2] = r.p.z, v[3] = r.p.w;
    } else if constexpr (MODE == A_BNRELU) {
        const float4 s = *reinterpret_cast<const float4 *>(A.scale + k);
        const float4 h = *reinterpret_cast<const float4 *>(A.shift + k);
        v[0] = fmaxf(fmaf(r.p.x, s.x, h.x), 0.f);
        v[1] = fmaxf(fmaf(r.p.y, s.y, h.y), 0.f);
        v[2] = fmaxf(fmaf(r.p.z, s.z, h.z), 0.f);
        v[3] = fmaxf(fmaf(r.p.w, s.w, h.w), 0.f);
    } else if constexpr (MODE == A_GATHER || MODE == A_CONCAT) {
        // float32 subtraction of the centre, pointnet_pp_8dir.py:32 (q = 0 for features and for group_all)
        v[0] = __fsub_rn(r.p.x, r.q.x), v[1] = __fsub_rn(r.p.y, r.q.y);
        v[2] = __fsub_rn(r.p.z, r.q.z), v[3] = __fsub_rn(r.p.w, r.q.w);
    } else {  // A_DZ / A_DZ_POOL
        float4 dy = r.p;
        if constexpr (MODE == A_DZ_POOL) {
            const int kk = row % A.K;  // neighbour slot of this row inside its group
            dy.x = kk == r.ia.x ? dy.x : 0.f, dy.y = kk == r.ia.y ? dy.y : 0.f;
            dy.z = kk == r.ia.z ? dy.z : 0.f, dy.w = kk == r.ia.w ? dy.w : 0.f;
        }
        const float *c = A.cst + k;
        const float4 g = *reinterpret_cast<const float4 *>(c);
        const float4 mu = *reinterpret_cast<const float4 *>(c + A.C);
        const float4 is = *reinterpret_cast<const float4 *>(c + 2 * A.C);
        const float4 c1 = *reinterpret_cast<const float4 *>(c + 3 * A.C);
        const float4 c2 = *reinterpret_cast<const float4 *>(c + 4 * A.C);
        v[0] = g.x * (dy.x - c1.x - (r.q.x - mu.x) * is.x * c2.x);
        v[1] = g.y * (dy.y - c1.y - (r.q.y - mu.y) * is.y * c2.y);
        v[2] = g.z * (dy.z - c1.z - (r.q.z - mu.z) * is.z * c2.z);
        v[3] = g.w * (dy.w - c1.w - (r.q.w - mu.w) * is.w * c2.w);
    }
}

// scalar flavour used by the dW kernel (one element per lane: the channel index sits on the lane, the
// per-channel constants are hoisted into registers once per wave)
struct ChanConst {
    float g, mu, is, c1, c2;  // A_DZ
    float sc, sh;             // A_BNRELU
};

template <int MODE>
__device__ __forceinline__ ChanConst load_chan_const(const AOperand &A, int k, int Kvalid) {
    ChanConst c{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k >= Kvalid) return c;
    if constexpr (MODE == A_DZ || MODE == A_DZ_POOL) {
        const float *p = A.cst + k;
        c.g = p[0], c.mu = p[A.C], c.is = p[2 * A.C], c.c1 = p[3 * A.C], c.c2 = p[4 * A.C];
    } else if constexpr (MODE == A_BNRELU) {
        c.sc = A.scale[k], c.sh = A.shift[k];
    }
    return c;
}

// raw loads of element (row, k): up to two values (second one: z for A_DZ*, centre coordinate for A_GATHER).
// Unconditional loads on clamped indices; xform_a1 masks what was out of range.
template <int MODE>
__device__ __forceinline__ float2 fetch_a1(const AOperand &A, int row, int k, int Kvalid, int M) {
    float2 r = make_float2(0.f, 0.f);
    const int rc = min(row, M - 1), kc = min(k, Kvalid - 1);
    if constexpr (MODE == A_PLAIN || MODE == A_BNRELU) {
        r.x = A.a[(size_t)rc * A.lda + kc];
    } else if constexpr (MODE == A_DZ) {
        r.x = A.a[(size_t)rc * A.lda + kc];
        r.y = A.z[(size_t)rc * A.lda + kc];
    } else if constexpr (MODE == A_DZ_POOL) {
        const int g = rc / A.K;
        const size_t gi = (size_t)g * A.lda + kc;
        const float d = A.a[gi];
        r.x = (rc - g * A.K == A.arg[gi]) ? d : 0.f;
        r.y = A.z[(size_t)rc * A.lda + kc];
    } else if constexpr (MODE == A_GATHER) {
        const int grp = rc / A.K;
        const size_t prow = (size_t)(grp / A.S) * A.N + A.idx[rc];
        const bool feat = kc < A.D;
        const int xc = min(max(kc - A.D, 0), 2);
        const float *src = feat ? A.a + prow * A.D + kc : A.xyz + prow * 3 + xc;
        r.x = *src;
        const float cv = A.new_xyz[(size_t)grp * 3 + xc];
        r.y = feat ? 0.f : cv;
    } else {  // A_CONCAT
        const bool feat = kc < A.D;
        const int xc = min(max(kc - A.D, 0), 2);
        const float *src = feat ? A.a + (size_t)rc * A.D + kc : A.xyz + (size_t)rc * 3 + xc;
        r.x = *src;
    }
    return r;
}

template <int MODE>
__device__ __forceinline__ float xform_a1(const float2 r, const ChanConst &c, int k, int Kvalid, bool ok) {
    // out-of-range lanes were loaded from clamped (valid, finite) addresses and are zeroed by a multiplication: a
    // select here lets hipcc sink the loads into a per-lane branch and wait for each of them separately
    const float m = (ok && k < Kvalid) ? 1.f : 0.f;
    if constexpr (MODE == A_PLAIN) {
        return r.x * m;
    } else if constexpr (MODE == A_BNRELU) {
        return fmaxf(fmaf(r.x, c.sc, c.sh), 0.f) * m;
    } else if constexpr (MODE == A_DZ || MODE == A_DZ_POOL) {
        return c.g * (r.x - c.c1 - (r.y - c.mu) * c.is * c.c2) * m;
    } else {
        return __fsub_rn(r.x, r.y) * m;
    }
}

}  // namespace pnpp
