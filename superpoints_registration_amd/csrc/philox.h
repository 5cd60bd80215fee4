// Philox4x32-10 and the (seed, pair_key, side, element, tag) block layout of the draw contracts in include/spr.h:
// one definition for augment.hip (tags 0, 1, 2), ransac.hip (tag 3) and modelnet_pairs.hip (tags 16-20), host and device.
#pragma once
#include <cstdint>

#include "spr_common.h"

namespace spr {

constexpr uint32_t kPhM0 = 0xD2511F53u, kPhM1 = 0xCD9E8D57u, kPhW0 = 0x9E3779B9u, kPhW1 = 0xBB67AE85u;

struct Philox4 {
  uint32_t w[4];
};

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kPhM0 * c0, p1 = (uint64_t)kPhM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kPhW0;
    k1 += kPhW1;
  }
  Philox4 o;
  o.w[0] = c0, o.w[1] = c1, o.w[2] = c2, o.w[3] = c3;
  return o;
}

// block (element, q = 2 pair_key + side, tag) of a seed
__host__ __device__ inline Philox4 philox_block(uint64_t seed, uint64_t pair_key, int side, uint32_t element,
                                                uint32_t tag) {
  const uint64_t q = 2 * pair_key + (uint64_t)side;
  return philox4x32_10(element, (uint32_t)q, tag, (uint32_t)(q >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

constexpr uint32_t kTagPair = 0, kTagNoise = 1, kTagKey = 2, kTagRansac = 3;
// 8f-7 (ModelNet pairs): pair decisions, resample keys, up-sampling extras, jitter noise, shuffle keys
constexpr uint32_t kTagMnPair = 16, kTagMnResample = 17, kTagMnExtra = 18, kTagMnNoise = 19, kTagMnShuffle = 20;

#ifdef __HIPCC__
// u(w) in float32 (exact: 24 significant bits)
__device__ __forceinline__ float philox_u32(uint32_t w) { return __fmul_rn((float)(w >> 9) + 0.5f, 1.1920928955078125e-7f); }

// The float32 normal triple of a block (8f-6): (r(w0) cos(w1), r(w0) sin(w1), r(w2) cos(w3)) with the accurate
// logf / sincosf / sqrtf, one rounding per operation
__device__ __forceinline__ void philox_normal3(const Philox4& b, float* n) {
  const float r0 = sqrtf(__fmul_rn(-2.f, logf(philox_u32(b.w[0]))));
  const float r1 = sqrtf(__fmul_rn(-2.f, logf(philox_u32(b.w[2]))));
  float s0, c0, s1, c1;
  sincosf(__fmul_rn(6.2831855f, philox_u32(b.w[1])), &s0, &c0);
  sincosf(__fmul_rn(6.2831855f, philox_u32(b.w[3])), &s1, &c1);
  n[0] = __fmul_rn(r0, c0);
  n[1] = __fmul_rn(r0, s0);
  n[2] = __fmul_rn(r1, c1);
}
#endif

}  // namespace spr
