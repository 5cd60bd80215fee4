// Philox4x32-10 and the (seed, pair_key, side, element, tag) block layout of the draw contracts in include/spr.h:
// one definition for augment.hip (tags 0, 1, 2) and ransac.hip (tag 3), host and device.
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

}  // namespace spr
