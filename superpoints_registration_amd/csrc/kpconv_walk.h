// The neighbour walk of the one-wave-per-row KPConv kernels (kpconv_modes.hip: rigid kernel points, every mode;
// kpconv_deform.hip: kernel points per query): a lane's neighbour load, the influence functions and the lane = channel
// accumulation over neighbours staged in LDS.  Each file stages the influences its own way.  Include after spr_common.h.
#pragma once
#include "spr_common.h"

namespace spr {
namespace {

constexpr int kWalkKP = 16;   // accumulators of a lane's walk: the most kernel points of the one-wave-per-query kernels
constexpr int kSlot = 16;     // floats per staged neighbour at most: SUM its influences, CLOSEST {influence, arg-min p}
constexpr int slot_floats(int agg) { return agg == SPR_KP_CLOSEST ? 2 : kSlot; }
constexpr int kBatch = 8;     // gathered feature values in flight per lane

template <int INFL>
__device__ __forceinline__ float influence_of(float d2, float inv_extent, float gauss_den) {
  if constexpr (INFL == SPR_KP_CONSTANT) {
    return 1.f;
  } else if constexpr (INFL == SPR_KP_LINEAR) {
    return fmaxf(0.f, 1.f - sqrtf(d2) * inv_extent);
  } else {
    static_assert(INFL == SPR_KP_GAUSSIAN, "influence");
    return expf(-d2 / gauss_den);
  }
}

// Lane = one neighbour of a query's row.  load_neighbour: its index (-1: shadow or past the row), its position relative
// to the query and its flag (flag == NULL: 0) -- loads without branches, so that a caller can issue several rows' before
// it uses the first.
struct KpNeighbour {
  int id;
  float px, py, pz;
  int pos;
};
__device__ __forceinline__ KpNeighbour load_neighbour(const int* __restrict__ nbr_row, int kk, int kmax, bool live,
                                                      const float* __restrict__ s_xyz, int ns, float qx, float qy,
                                                      float qz, const unsigned char* __restrict__ flag) {
  const int raw = kk < kmax ? nbr_row[kk] : -1;
  const bool ok = live && raw >= 0 && raw < ns;
  const size_t sid = ok ? (size_t)raw : 0;          // row 0 exists (ns > 0); what it gives is not used
  KpNeighbour nb;
  nb.id = ok ? raw : -1;
  nb.px = s_xyz[3 * sid] - qx;
  nb.py = s_xyz[3 * sid + 1] - qy;
  nb.pz = s_xyz[3 * sid + 2] - qz;
  nb.pos = flag != nullptr ? (int)flag[sid] : 0;
  return nb;
}

// Lane = channel: acc[p] += influence[k][p] * x[ids[k]][channel] over the nv staged neighbours, kBatch gathers in
// flight.  xcol = x + the lane's channel (cok: the lane has one).  HALF: the half-waves take the even / odd staged
// neighbours (the caller adds the halves).  constant / sum keeps ONE sum, in acc[0].
// closest is a sparse accumulate -- a neighbour's row goes to ONE kernel point's slot, and the accumulators stay in
// registers: a whole wave walks one neighbour at a time, so the arg-min is wave uniform and a scalar branch leads to
// one add; the half-waves of HALF hold two neighbours, there 15 selects.  (A wave-private float table in LDS with one
// ds_add_f32 per neighbour and lane was measured at 1.8x the time of this form: profiles/kpconv_modes_bench.txt.)
template <int INFL, int AGG, bool HALF>
__device__ __forceinline__ void walk_neighbours(const float* __restrict__ xcol, bool cok, int cin, int nv,
                                                const float* __restrict__ infl, const int* __restrict__ ids,
                                                int half, float (&acc)[kWalkKP]) {
  constexpr int SLOT = slot_floats(AGG);
  constexpr int STEP = HALF ? 2 : 1;
  constexpr int NB = HALF ? kBatch / 2 : kBatch;   // per lane; a wave has kBatch neighbours in flight either way
  for (int k0 = 0; k0 < nv; k0 += NB * STEP) {
    float xv[NB];
    int ks[NB];
    float2 wp[NB];                                        // closest: {influence, arg-min p} of the batch, read
#pragma unroll                                                // ahead so that no branch below waits for LDS
    for (int b = 0; b < NB; ++b) {
      const int k = k0 + b * STEP + half;
      const bool valid = k < nv;
      ks[b] = valid ? k : 0;                                  // slot 0 exists (nv > 0); its value is masked
      const int id = ids[ks[b]];
      if constexpr (AGG == SPR_KP_CLOSEST) wp[b] = *reinterpret_cast<const float2*>(infl + ks[b] * SLOT);
      xv[b] = (valid && cok) ? xcol[(size_t)id * cin] : 0.f;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (!HALF && k0 + b >= nv) break;                       // wave uniform
      const float* iw = infl + ks[b] * SLOT;
      if constexpr (AGG == SPR_KP_CLOSEST) {
        const float v = wp[b].x * xv[b];
        if constexpr (HALF) {
          const int pm = __float_as_int(wp[b].y);
#pragma unroll
          for (int p = 0; p < kWalkKP; ++p) acc[p] += p == pm ? v : 0.f;
        } else {
          // one staged neighbour per step: the index is wave uniform and the register array is indexed through M0
          acc[__builtin_amdgcn_readfirstlane(__float_as_int(wp[b].y)) & (kWalkKP - 1)] += v;
        }
      } else if constexpr (INFL == SPR_KP_CONSTANT) {
        acc[0] += xv[b];
      } else {
#pragma unroll
        for (int p4 = 0; p4 < kWalkKP / 4; ++p4) {
          const float4 v = *reinterpret_cast<const float4*>(iw + 4 * p4);
          acc[4 * p4] += v.x * xv[b];
          acc[4 * p4 + 1] += v.y * xv[b];
          acc[4 * p4 + 2] += v.z * xv[b];
          acc[4 * p4 + 3] += v.w * xv[b];
        }
      }
    }
  }
}

}  // namespace
}  // namespace spr
