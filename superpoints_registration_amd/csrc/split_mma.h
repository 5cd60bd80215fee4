// Split-fp16 matrix products: the vector types, the three-MFMA product, the accumulator row maps and the staging of
// hi / lo planes -- the matrix half of the idea whose scalar half (split_pk_s, pow2_exp_for, block_absmax) is in
// spr_common.h.  Include after spr_common.h.  The only place the fp16 MFMA builtins exist.
//
// Operand split and scale.  Each operand tensor x is multiplied by a per-tensor power of two s_x that brings max |x|
//   into [2^14, 2^15) (max |x| from a pre-pass: launch_absmax -> partials, reduced in the consumer's prologue:
//   ka = pow2_exp_for(block_absmax(a_parts ..)), kb likewise, s_a = pow2f(ka), s_b = pow2f(kb)), then split:
//   x s_x = hi + lo, hi = fp16(x s_x), lo = fp16(x s_x - hi) (split_pk_s).  No operand can overflow fp16; every element
//   within 2^-18 of its tensor's maximum keeps 22 significand bits, smaller ones an absolute error of 2^-39 max |x|.
//     a.b ~= (ah.bh + ah.bl + al.bh) / (s_a s_b)          (al.bl ~ 2^-22 |a.b| dropped)
//   The matrix cores honour fp16 subnormals on both operands (scripts/abl/denorm.hip), products are exact and accumulate
//   in fp32, so all three share ONE fp32 accumulator; the epilogue multiplies by the exact pow2f(-ka - kb).
//   Three fp16 MFMAs per k-step replace eight exact-f32 ones of twice the length (1/5 of the matrix-pipe time).
// Term order.  Small terms first, then the dominant one: A.hi B.lo, A.lo B.hi, A.hi B.hi (A / B = first / second MFMA
//   operand).  fp32 accumulation is not associative, so the order is part of the result's bits.  A site that computes
//   the TRANSPOSED product (operands swapped, C^T in the accumulator) and must keep the bits of the untransposed one
//   asks for mma3_*<true>: A.lo B.hi, A.hi B.lo, A.hi B.hi.
// Fragments (wave of 64 lanes, 8 consecutive k per lane in one f16x8).
//   32x32x16: lane l holds row (A) / column (B)  l & 31,  k = 8 (l >> 5) + 0..7.
//     C: f32x16, lane column l & 31, register r = row acc_row32(r, l >> 5) = (r & 3) + 8 (r >> 2) + 4 (l >> 5).
//     Registers 8 s .. 8 s + 7 of a C tile are therefore the B fragment of k-step s of a product that contracts over
//     the tile's rows, in the row order 16 s + 8 (j >> 2) + 4 (l >> 5) + (j & 3), j = 0..7.
//   16x16x32: lane l holds row / column  l & 15,  k = 8 (l >> 4) + 0..7.
//     C: f32x4, lane column l & 15, register r = row acc_row16(r, l >> 4) = 4 (l >> 4) + r.
// Planes in LDS.  A staged [rows][32 k] slab is two fp16 planes (hi, lo) with a row stride of kPlaneStride = 40 halves
//   (32 + 8 pad = 80 bytes, rows stay 16-byte aligned).  The 16 bytes a lane reads from row r start at bank
//   20 r mod 64 = 4 (5 r mod 16); 5 is odd, so any 16 rows that differ mod 16 -- each lane group of a ds_read_b128 --
//   cover the 64 banks once: fragment reads (frag_ld40) are conflict-free.
#pragma once
#include "spr_common.h"

namespace spr {
#ifdef __HIPCC__

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- the product -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x16 mma1_32(const f16x8& a, const f16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
template <bool TRANSPOSED = false>
__device__ __forceinline__ f32x16 mma3_32(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x16 c) {
  f32x16 d = __builtin_amdgcn_mfma_f32_32x32x16_f16(TRANSPOSED ? al : ah, TRANSPOSED ? bh : bl, c, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_32x32x16_f16(TRANSPOSED ? ah : al, TRANSPOSED ? bl : bh, d, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, d, 0, 0, 0);
}
template <bool TRANSPOSED = false>
__device__ __forceinline__ f32x4 mma3_16(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x4 c) {
  f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_f16(TRANSPOSED ? al : ah, TRANSPOSED ? bh : bl, c, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_f16(TRANSPOSED ? ah : al, TRANSPOSED ? bl : bh, d, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, d, 0, 0, 0);
}

// ---- accumulator row maps (lh = lane >> 5, kg = lane >> 4) -----------------------------------------------------------
// Integer sums reach the address code in the order they are written, so there are two spellings of the one map:
// x + acc_row32(r, lh) adds the row as one term; acc_row32(r, lh, base) adds its terms to `base` from left to right.
__device__ __forceinline__ int acc_row32(int r, int lh) { return 8 * (r >> 2) + 4 * lh + (r & 3); }
__device__ __forceinline__ int acc_row32(int r, int lh, int base) { return base + (r & 3) + 8 * (r >> 2) + 4 * lh; }
__device__ __forceinline__ int acc_row16(int r, int kg) { return 4 * kg + r; }

// ---- four consecutive values: split, then 8 bytes into a hi and into a lo plane (8-byte aligned) ----------------------
__device__ __forceinline__ void split_store4(const f32x4& v, float s, _Float16* hi, _Float16* lo) {
  unsigned int h0, h1, l0, l1;
  split_pk_s(v[0], v[1], s, h0, l0);
  split_pk_s(v[2], v[3], s, h1, l1);
  *reinterpret_cast<u32x2*>(hi) = (u32x2){h0, h1};
  *reinterpret_cast<u32x2*>(lo) = (u32x2){l0, l1};
}
__device__ __forceinline__ void split_store4(const float4& v, float s, _Float16* hi, _Float16* lo) {
  split_store4((f32x4){v.x, v.y, v.z, v.w}, s, hi, lo);
}

// ---- 40-half planes --------------------------------------------------------------------------------------------------
constexpr int kPlaneK = 32;        // k per staged slab
constexpr int kPlaneStride = 40;   // row stride in halves
// the lane's fragment of k-step ko / 16 of `row`: ko = 16 s + 8 (lane >> 5)
__device__ __forceinline__ void frag_ld40(const _Float16* hi_plane, const _Float16* lo_plane, int row, int ko, f16x8& h,
                                          f16x8& l) {
  h = *reinterpret_cast<const f16x8*>(hi_plane + row * kPlaneStride + ko);
  l = *reinterpret_cast<const f16x8*>(lo_plane + row * kPlaneStride + ko);
}

// Slab staging of the NT split GEMM  C[BM x BN] += X[BM rows][32 k] . W[BN rows][32 k]^T, one operand per call: NT
// threads carry ROWS * 8 / NT float4 each of the next slab in registers (slab_load), then scale, split and store them
// into the operand's two planes (slab_store).  No waits and no barriers in here: slab_load issues asm loads the compiler
// does not count; the caller retires them (wait_vm, lds_dma.h) before slab_store and places its own barriers.
// The caller's variables come by reference, as a lambda captures them (by value the address code compiles differently).
//
// rows row0.. of X [M, K], columns k0 .. k0 + 31.  Rows past M are clamped: they produce finite garbage in accumulator
// rows / columns that the epilogue never writes.
template <int ROWS, int NT, typename Ptr>
__device__ __forceinline__ void slab_load(f32x4 (&regs)[ROWS * (kPlaneK / 4) / NT], const Ptr& X, const int& M,
                                          const int& K, const int& tid, int row0, int k0) {
  static_assert(ROWS * (kPlaneK / 4) % NT == 0, "slab must divide over the threads");
#pragma unroll
  for (int i = 0; i < ROWS * (kPlaneK / 4) / NT; ++i) {
    const int f = tid + i * NT;
    const int r = f / (kPlaneK / 4), c4 = f % (kPlaneK / 4);
    const float* p = X + (size_t)min(row0 + r, M - 1) * K + k0 + c4 * 4;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(regs[i]) : "v"(p));
  }
}
template <int ROWS, int NT>
__device__ __forceinline__ void slab_store(const f32x4 (&regs)[ROWS * (kPlaneK / 4) / NT], const float& s,
                                           _Float16* const& hi_plane, _Float16* const& lo_plane, const int& tid) {
#pragma unroll
  for (int i = 0; i < ROWS * (kPlaneK / 4) / NT; ++i) {
    const int f = tid + i * NT;
    const int r = f / (kPlaneK / 4), c4 = f % (kPlaneK / 4);
    split_store4(regs[i], s, hi_plane + r * kPlaneStride + c4 * 4, lo_plane + r * kPlaneStride + c4 * 4);
  }
}

#endif
}  // namespace spr
