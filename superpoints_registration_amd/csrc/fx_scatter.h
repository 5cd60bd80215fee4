// Order-independent scatter-adds: the 64-bit fixed-point accumulation of the backward's scatters (backward.hip:
// max-pool, row gather, the KPConv neighbour gather; kpconv_modes.hip: the mode-aware KPConv gather), their scratch
// layout and the conversion back to float.  Include after spr_common.h.
#pragma once
#include "spr_common.h"

namespace spr {
namespace {

#ifdef __HIPCC__
// ---- order-independent scatter-adds ----------------------------------------------------------------
// Several queries send a contribution to the same (row, channel) of a gradient (max-pool, row gather, the
// KPConv's neighbour gather).  Float atomics made those sums depend on the arrival order (run-to-run
// differences at rounding level).  Here a contribution is converted to 64-bit FIXED POINT -- scaled by a
// power of two 2^fx derived from the measured maximum of the incoming gradient, so that the largest
// contribution sits near 2^40 -- and added with integer atomics: integer addition is associative, the
// result does not depend on the order.  Resolution 2^-40 of the largest contribution (finer than the
// 2^-24 of a float running sum); 2^22 maximal contributions fit before overflow.  k_fx_to_float converts.
//
// The exponent is NOT pow2_exp_for's (clamped to +-60 for the split-fp16 planes): a clamp left gradients below
// ~2^-46 with fewer than 40 bits (every contribution rounded to 0 below ~2^-85) and overflowed the 64-bit sums
// above ~2^74.  fx_exp_for is exact for every finite positive bound amax * factor (denormals and results
// beyond float range included): fx lies in [-93, 188], so fx / 2 and fx - fx / 2 are valid pow2f exponents.
// Where pow2_exp_for is not clamped (bounds in [2^-46, 2^75)) the two agree, and so do the sums, bit for bit.
__device__ __forceinline__ int fx_exp_for(float amax, float factor) {
  if (!(amax > 0.f) || !(amax < 3.0e38f)) return 0;
  int e1, e2;
  const float m = frexpf(amax, &e1);            // amax = m 2^e1, m in [0.5, 1): exact, denormals included
  frexpf(m * factor, &e2);                      // factor > 0: amax * factor in [2^(e1+e2-1), 2^(e1+e2))
  return 40 - (e1 + e2);                        // max |v| 2^fx in [2^39, 2^40)
}
__device__ __forceinline__ int fx_exp(const float* __restrict__ parts, float* sh, float factor) {
  return fx_exp_for(block_absmax(parts, sh), factor);
}
__device__ __forceinline__ void fx_add(unsigned long long* acc, float v, int fx) {
  // v * 2^fx exactly (two exact power-of-two factors keep the intermediate in float range)
  const float sc = (v * pow2f(fx / 2)) * pow2f(fx - fx / 2);
  atomicAdd(acc, (unsigned long long)__float2ll_rn(sc));
}
__global__ void k_fx_to_float(const unsigned long long* __restrict__ acc, long n, const float* __restrict__ parts,
                              float factor, float* __restrict__ out) {
  __shared__ float sh[17];
  const float amax = block_absmax(parts, sh);
  const int fx = fx_exp_for(amax, factor);
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!(amax < 3.0e38f)) {   // the incoming gradient holds an inf or a NaN (k_absmax maps NaN to inf): a float
    out[i] = __builtin_nanf("");   // atomicAdd would have propagated it; the fixed-point sums cannot, so the
    return;                        // whole gradient is marked (a finite-gradient check downstream still fires)
  }
  const double inv = (double)pow2f(-(fx / 2)) * (double)pow2f(-(fx - fx / 2));
  out[i] = (float)((double)(long long)acc[i] * inv);
}
// an externally published range (n partials) as the kAmaxParts partials the fixed-point kernels read
__global__ __launch_bounds__(256) void k_range_to_parts(const float* __restrict__ range, int n, float* __restrict__ parts) {
  __shared__ float sh[17];
  const float m = block_absmax(range, sh, n);
  for (int i = threadIdx.x; i < kAmaxParts; i += 256) parts[i] = i == 0 ? m : 0.f;
}
#endif

// scratch of the order-independent scatter-adds: the fixed-point accumulators + the range partials of the
// incoming gradient
struct FxScratch {
  unsigned long long* acc;
  float* parts;
};
inline FxScratch fx_layout(Workspace& w, long rows, int c) {
  FxScratch f;
  f.acc = w.take<unsigned long long>((size_t)(rows > 0 ? rows : 1) * (size_t)(c > 0 ? c : 1));
  f.parts = w.take<float>(kAmaxParts);
  return f;
}
inline int fx_scratch(void* ws, size_t ws_bytes, long rows, int c, hipStream_t stream, FxScratch* out) {
  Workspace w(ws, ws_bytes);
  *out = fx_layout(w, rows, c);
  SPR_REQUIRE(ws != nullptr && w.ok(), "scatter: workspace too small");
  SPR_HIP_CHECK(hipMemsetAsync(out->acc, 0, (size_t)rows * c * sizeof(unsigned long long), stream));
  return 0;
}

}  // namespace
}  // namespace spr
