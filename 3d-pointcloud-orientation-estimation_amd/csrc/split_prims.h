// split_prims.h -- the device primitives every split-product kernel shares, ONE definition: the exact three-way split of float32 into
// bfloat16 pieces, the MFMA operand casts, the transposed LDS read, the row swizzle of the plane images, the raw buffer loads
// and the stores with a cache policy.  A new kernel includes this header; it does not paste from another kernel.
//
// Why.  gfx950 has no reduced-width float32 MFMA: v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 rate (64 FLOP/clk/SIMD), and on the
// float32 forward kernels the MFMA time and the HBM time ADD.  A float32 number is the exact sum of three
// bfloat16 numbers (24 significand bits = 8 + 8 + 8; bf16 has float32's exponent range):
//     a = a_h + a_m + a_l,   a_h = bf16(a),  a_m = bf16(a - a_h),  a_l = a - a_h - a_m   (every subtraction exact, a_l exact in bf16)
// so  a b = a_h b_h + (a_h b_m + a_m b_h) + (a_h b_l + a_l b_h + a_m b_m) + [a_m b_l + a_l b_m + a_l b_l].
// The bracket is at most 2^-25 |a b| -- below the rounding of the float32 accumulation itself (2^-24 per addition) -- and is dropped; the
// six products kept are exact in float32 (8 x 8 significand bits) and are accumulated in float32 by v_mfma_f32_32x32x16_bf16: six
// instructions of 32 cycles for 16 reduction steps against eight of 64 cycles = 2.67 x the float32 MFMA rate.  The leading products go
// to one accumulator and the five small ones to a second, added once per strip, so the rounding of the sum is that of a float32
// accumulation of the leading products.  (Why two accumulators: v_mfma_f32_32x32x16_bf16 aligns its 16 products and the accumulator to
// the largest exponent among them and drops what lies 2^-26 below it -- tools/mfma_round.hip -- so small addends must not meet the
// large sum inside the instruction.)  Not a reduced-precision mode: tests/test_gpu_levels_routed.py holds it to the same gates as the
// float32 MFMA form, and tests/test_gpu_split_products.py measures both against float64.  (Infinities do not survive the split:
// inf - inf; the float32 form gives inf where this one gives NaN.  Operands below 2^-110 lose their low pieces to underflow.)
//
// Everything here is internal to the translation unit that includes it (anonymous namespace) and carries no pragma: each kernel file
// keeps its own compile flags.
#pragma once
#include <type_traits>

#include "common.h"

namespace pnpp {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---- the split: v = h + m + l, values packed two per dword (low half first) -----------------------------------------------------
__device__ __forceinline__ unsigned sp_pk(float lo, float hi) {   // two floats -> two bf16 in one dword, round to nearest even
    const f32x2v v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2v));
}
__device__ __forceinline__ float sp_lo(unsigned p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float sp_hi(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
// two floats -> their three bf16 pieces, two per dword
__device__ __forceinline__ void sp_split2(float v0, float v1, unsigned &h, unsigned &m, unsigned &l) {
    h = sp_pk(v0, v1);
    float r0 = v0 - sp_lo(h), r1 = v1 - sp_hi(h);
    m = sp_pk(r0, r1);
    r0 -= sp_lo(m), r1 -= sp_hi(m);
    l = sp_pk(r0, r1);
}
// four floats -> their three bf16 pieces, four per 8-byte word.  The statements are interleaved (all four conversions, then all four
// residuals, ...) and NOT two sp_split2 calls: the arithmetic is the same, the instruction schedule of the callers is not.
__device__ __forceinline__ void sp_split4(const f32x4 v, uint2 &h, uint2 &m, uint2 &l) {
    h.x = sp_pk(v[0], v[1]), h.y = sp_pk(v[2], v[3]);
    float r0 = v[0] - sp_lo(h.x), r1 = v[1] - sp_hi(h.x), r2 = v[2] - sp_lo(h.y), r3 = v[3] - sp_hi(h.y);
    m.x = sp_pk(r0, r1), m.y = sp_pk(r2, r3);
    r0 -= sp_lo(m.x), r1 -= sp_hi(m.x), r2 -= sp_lo(m.y), r3 -= sp_hi(m.y);
    l.x = sp_pk(r0, r1), l.y = sp_pk(r2, r3);
}

// ---- MFMA operands ---------------------------------------------------------------------------------------------------------------
// 16 bytes of one plane as the eight-element operand of v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ bf16x8 sp_op(uint4 v) { return __builtin_bit_cast(bf16x8, v); }
// four packed pairs of one plane, as sp_split2 leaves them, as the eight-element MFMA fragment (element 2 i = low half of p[i])
__device__ __forceinline__ bf16x8 sp_frag(const unsigned (&p)[4]) {
    const uint4 v = make_uint4(p[0], p[1], p[2], p[3]);
    return __builtin_bit_cast(bf16x8, v);
}

// ---- plane images in LDS -------------------------------------------------------------------------------------------------------
// ds_read_b64_tr_b16: 4 rows x 16 columns per 16 lanes, transposed
__device__ __forceinline__ uint2 sp_tr_b64(const unsigned char *p) {
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(p));
    return __builtin_bit_cast(uint2, v);
}
// Row swizzle of a plane image ([rows][64 k] bf16, 128-byte rows): 16-byte group g of row r sits at g ^ x(r), x(r) = 4 bit1(r) +
// bits3:2(r).  Conflict-free for the row reads (the four 16-lane groups of a ds_read_b128 see eight different x per row parity and
// touch all 64 banks once) and for the transposed reads (rows r and r + 2 of a block differ in x's bit 2); row rb + 4 i of the
// staging map (rb < 4) is one register ^ ((i & 3) << 4) + 512 i.  The writer and every reader of an image must use this one map.
__device__ __forceinline__ constexpr int sp_swz_row(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }

// ---- raw buffer loads ------------------------------------------------------------------------------------------------------------
// Raw (stride 0) resource of `records` bytes at `base`.  sp_buf_rsrc: the largest range, the callers keep their offsets inside their
// arrays; sp_buf_rsrc_null: zero bytes, every load returns 0 without touching memory -- what a fetch past the last strip is pointed at.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sp_buf_rsrc_n(const void *base, unsigned records) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, records, 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sp_buf_rsrc(const void *base) { return sp_buf_rsrc_n(base, 0xfffffffe); }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sp_buf_rsrc_null(const void *base) { return sp_buf_rsrc_n(base, 0); }
__device__ __forceinline__ f32x4 sp_buf_load4(__amdgpu_buffer_rsrc_t r, unsigned lane_off, unsigned s_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)lane_off, (int)s_off, 0));
}
__device__ __forceinline__ float sp_buf_load1(__amdgpu_buffer_rsrc_t r, unsigned lane_off, unsigned s_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)lane_off, (int)s_off, 0));
}

// ---- stores with a cache policy --------------------------------------------------------------------------------------------------
// A store is plain (write-back: the line stays dirty in the writing XCD's L2 until the launch ends) or write-through (sc1: the bytes
// leave for memory as they are stored, the line is not kept).  `wt` is uniform -- one bit of the launch's policy mask
// (pnpp_set_store_policy; common.h: StorePolicy), tested against the class of the site -- so the choice is a scalar branch, never per lane.
// A block of stores takes the branch ONCE, around the whole block (sp_with_policy: the flag becomes a compile-time constant inside, each
// side schedules as if the other did not exist); a branch per store inside an epilogue cost gemm_wsd3_kernel<128,32,A5> 7 us of its 39.  Values and order of the stores are the same in both forms: a policy changes no result.  Visibility stays
// the kernel boundary's; nothing inside a launch may read what these stores wrote.
// Forms: <= 8 bytes per lane a relaxed agent-scope atomic store on a global-address-space pointer (global_store ... sc1), buffer stores
// by the aux immediate (16 = sc1).  Never nt: it is slower on every stored edge and is not write-through.
template <typename F>
__device__ __forceinline__ void sp_with_policy(bool wt, F &&f) {   // f(std::true_type) or f(std::false_type): `wt` as a constant
    if (wt) f(std::true_type{});
    else f(std::false_type{});
}
template <typename T>
__device__ __forceinline__ void sp_store(T *p, T v, bool wt) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one dword or two per lane");
    typedef __attribute__((address_space(1))) T gT;
    if (wt) __hip_atomic_store((gT *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
__device__ __forceinline__ void sp_buf_store1(float v, __amdgpu_buffer_rsrc_t r, unsigned lane_off, unsigned s_off, bool wt) {
    if (wt) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)lane_off, (int)s_off, 16);
    else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)lane_off, (int)s_off, 0);
}

}  // namespace
}  // namespace pnpp
