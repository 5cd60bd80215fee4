// RANSAC over the correspondences of all pairs of a batch on gfx950 (RegTR.ransac, qk_regtr_full.py:400-421): n_hyp
// random `sample`-point subsets with replacement per pair, a weighted Procrustes solve on each, the hypothesis with
// the lowest mean residual over ALL of the pair's correspondences wins.  The contract (draws, summation order, the
// arg-min rule) is in include/spr.h ("RANSAC for all pairs"); this file follows it operation for operation.
//
// Two launches for the whole batch, no workspace, no atomics:
//   k_ransac_hyp   grid (ceil(n_hyp / 4), npairs) x 256 threads, ONE WAVE PER HYPOTHESIS: draw (inline Philox) or read
//                  the sample indices, gather the triples (a few KB per pair: they stay in L2), reduce the sums in
//                  float64 by wave shuffles, solve, round the pose to float32, store it, and score it over the pair's n
//                  entries in spr_pose_scores' arithmetic -- the pose never leaves registers in between.
//                  The butterfly leaves every sum in every lane, so every lane runs the same serial 3x3 solve on the
//                  same numbers: the SIMD executes it once either way, and the pose needs no hand-over to the lanes
//                  that score with it.
//   k_ransac_pick  one wave per pair: the first minimum of the scores (NaN never wins), the pose copy, the status.
// Nothing of a pair is staged in LDS, so a pair's size is bounded by the packing only.
#include "philox.h"
#include "procrustes_solve.h"
#include "spr_common.h"

namespace spr {
namespace {

// wave-uniform: set_cu[0] == 0 and set_cu ascending over all npairs + 1 entries
__device__ __forceinline__ bool ransac_layout_ok(const int* __restrict__ set_cu, int npairs, int lane) {
  bool bad = set_cu[0] != 0;
  for (int i = lane; i < npairs; i += 64) bad |= set_cu[i] > set_cu[i + 1];
  return __ballot(bad) == 0;
}

__host__ __device__ inline uint32_t ransac_index(uint32_t word, uint32_t n) {
  return (uint32_t)(((uint64_t)word * n) >> 32);
}

// sample s of hypothesis h: word s & 3 of block h * SB + (s >> 2) of the pair's tag-3 stream
__host__ __device__ inline uint32_t ransac_draw_one(uint64_t seed, uint64_t pair_key, uint32_t h, uint32_t sb, int s,
                                                    uint32_t n) {
  const Philox4 blk = philox_block(seed, pair_key, 0, h * sb + (uint32_t)(s >> 2), kTagRansac);
  const int k = s & 3;
  const uint32_t word = k == 0 ? blk.w[0] : k == 1 ? blk.w[1] : k == 2 ? blk.w[2] : blk.w[3];
  return ransac_index(word, n);
}

template <bool kDraw>
__global__ __launch_bounds__(256) void k_ransac_hyp(const float* __restrict__ a, const float* __restrict__ b,
                                                    const float* __restrict__ w, const int* __restrict__ set_cu,
                                                    int npairs, int n_hyp, int sample, uint64_t seed,
                                                    const uint64_t* __restrict__ pair_key,
                                                    const int* __restrict__ idx, float* __restrict__ score,
                                                    float* __restrict__ hyp_pose) {
  const int lane = threadIdx.x & 63;
  const int h = blockIdx.x * 4 + (threadIdx.x >> 6), pr = blockIdx.y;
  if (h >= n_hyp) return;                                   // whole waves leave: no barrier below
  if (!ransac_layout_ok(set_cu, npairs, lane)) return;      // k_ransac_pick reports it
  const int beg = set_cu[pr], n = set_cu[pr + 1] - beg;
  if (n == 0) return;
  const float* pa = a + 3 * (size_t)beg;
  const float* pb = b + 3 * (size_t)beg;
  const float* pw = w + beg;
  const size_t slot = (size_t)pr * n_hyp + h;
  const int* my_idx = kDraw ? nullptr : idx + slot * sample;
  const uint64_t key = kDraw ? pair_key[pr] : 0;
  const uint32_t sb = (uint32_t)(sample + 3) >> 2;
  auto pick = [&](int s) -> int {
    if (kDraw) return (int)ransac_draw_one(seed, key, (uint32_t)h, sb, s, (uint32_t)n);
    const int i = my_idx[s];
    return (unsigned)i < (unsigned)n ? i : 0;              // SPR_RANSAC_BAD_INDEX: taken as 0, never a wild read
  };

  // compute_rigid_transform in procrustes_solve.h's arithmetic; lane l sums samples l, l + 64, ... ascending
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};                    // sum w, sum w*a (3), sum w*b (3)
  for (int s = lane; s < sample; s += 64) {
    const int i = pick(s);
    const double wi = (double)pw[i];
    acc[0] += wi;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      acc[1 + d] += wi * (double)pa[3 * (size_t)i + d];
      acc[4 + d] += wi * (double)pb[3 * (size_t)i + d];
    }
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) acc[k] = wave_sum_d(acc[k]);
  const double den = fmax(acc[0], 1e-6);                    // clamp_min(sum w, 1e-6)
  double ca[3], cb[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    ca[d] = acc[1 + d] / den;
    cb[d] = acc[4 + d] / den;
  }
  double cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int s = lane; s < sample; s += 64) {
    const int i = pick(s);
    const double wi = (double)pw[i] / den;
    double da[3], db[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      da[d] = (double)pa[3 * (size_t)i + d] - ca[d];
      db[d] = ((double)pb[3 * (size_t)i + d] - cb[d]) * wi;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) cov[3 * r + c] += da[r] * db[c];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) cov[k] = wave_sum_d(cov[k]);
  float T[12];
  procrustes_pose(cov, ca, cb, T);                          // every lane: the same numbers, the same pose
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) hyp_pose[12 * slot + k] = T[k];
  }

  // k_pose_scores (match_pose.hip), expression for expression
  float sum = 0.f;
  for (int i = lane; i < n; i += 64) {
    const float x = pa[3 * (size_t)i], y = pa[3 * (size_t)i + 1], z = pa[3 * (size_t)i + 2];
    float d2 = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float v = pb[3 * (size_t)i + r] - ((x * T[4 * r] + y * T[4 * r + 1] + z * T[4 * r + 2]) + T[4 * r + 3]);
      d2 += v * v;
    }
    sum += sqrtf(d2);
  }
  sum = wave_sum(sum);
  if (lane == 0) score[slot] = sum / (float)n;
}

// best = 0; for h = 1 .. n_hyp - 1: if (score[h] < score[best]) best = h -- as a wave arg-min: the lowest index among
// the smallest non-NaN scores, and 0 when score[0] is NaN (nothing compares below a NaN)
__global__ __launch_bounds__(64) void k_ransac_pick(const int* __restrict__ set_cu, int npairs, int n_hyp, int sample,
                                                    const int* __restrict__ idx, const float* __restrict__ score,
                                                    const float* __restrict__ hyp_pose, float* __restrict__ pose,
                                                    int* __restrict__ best, int* __restrict__ status) {
  const int lane = threadIdx.x, pr = blockIdx.x;
  float* po = pose + 12 * (size_t)pr;
  if (!ransac_layout_ok(set_cu, npairs, lane)) {
    if (lane < 12) po[lane] = 0.f;
    if (lane == 0) status[pr] = SPR_RANSAC_BAD_LAYOUT;
    return;
  }
  const int n = set_cu[pr + 1] - set_cu[pr];
  if (n == 0) {
    if (lane < 12) po[lane] = (lane == 0 || lane == 5 || lane == 10) ? 1.f : 0.f;
    if (lane == 0) {
      best[pr] = -1;
      status[pr] = SPR_RANSAC_EMPTY;
    }
    return;
  }
  bool bad = false;
  if (idx != nullptr) {
    const int* p = idx + (size_t)pr * n_hyp * sample;
    const size_t total = (size_t)n_hyp * sample;
    for (size_t k = lane; k < total; k += 64) bad |= (unsigned)p[k] >= (unsigned)n;
  }
  const bool any_bad = __ballot(bad) != 0;
  const float* sc = score + (size_t)pr * n_hyp;
  constexpr int kNone = 0x7fffffff;
  float bs = 0.f;
  int bh = kNone;
  for (int h = lane; h < n_hyp; h += 64) {
    const float c = sc[h];
    if (c == c && (bh == kNone || c < bs)) {
      bs = c;
      bh = h;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o, 64);
    const int oh = __shfl_xor(bh, o, 64);
    if (oh != kNone && (bh == kNone || os < bs || (os == bs && oh < bh))) {
      bs = os;
      bh = oh;
    }
  }
  const float s0 = sc[0];
  if (s0 != s0 || bh == kNone) bh = 0;
  if (lane < 12) po[lane] = hyp_pose[12 * ((size_t)pr * n_hyp + bh) + lane];
  if (lane == 0) {
    best[pr] = bh;
    status[pr] = any_bad ? SPR_RANSAC_BAD_INDEX : 0;
  }
}

int ransac_check_sizes(const char* what, int npairs, int n_hyp, int sample) {
  SPR_REQUIRE(npairs >= 0, "%s: negative npairs %d", what, npairs);
  SPR_REQUIRE(n_hyp >= 1 && sample >= 1, "%s: n_hyp %d and sample %d must be at least 1", what, n_hyp, sample);
  SPR_REQUIRE((uint64_t)n_hyp * (uint64_t)((sample + 3LL) / 4) < (1ull << 32),
              "%s: n_hyp * ceil(sample / 4) = %d * %lld does not fit the 32-bit block counter", what, n_hyp,
              (sample + 3LL) / 4);
  return 0;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" int spr_ransac_draw(uint64_t seed, const uint64_t* pair_key_host, const int* n_host, int npairs, int n_hyp,
                               int sample, int* idx_host) {
  if (int rc = ransac_check_sizes("ransac_draw", npairs, n_hyp, sample)) return rc;
  if (npairs == 0) return 0;
  SPR_REQUIRE(pair_key_host && n_host && idx_host, "ransac_draw: null pointer");
  for (int p = 0; p < npairs; ++p) {
    SPR_REQUIRE(pair_key_host[p] < (1ull << 63), "ransac_draw: pair_key[%d] must be below 2^63", p);
    SPR_REQUIRE(n_host[p] >= 0, "ransac_draw: n[%d] = %d is negative", p, n_host[p]);
  }
  const uint32_t sb = (uint32_t)((sample + 3LL) / 4);
  for (int p = 0; p < npairs; ++p)
    for (int h = 0; h < n_hyp; ++h) {
      int* out = idx_host + ((size_t)p * n_hyp + h) * sample;
      for (int s = 0; s < sample; ++s)
        out[s] = (int)ransac_draw_one(seed, pair_key_host[p], (uint32_t)h, sb, s, (uint32_t)n_host[p]);
    }
  return 0;
}

extern "C" int spr_ransac_pairs(const float* a, const float* b, const float* w, const int* set_cu, int npairs,
                                int n_hyp, int sample, uint64_t seed, const uint64_t* pair_key, const int* idx,
                                float* pose, int* best, float* score, float* hyp_pose, int* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = ransac_check_sizes("ransac_pairs", npairs, n_hyp, sample)) return rc;
  if (npairs == 0) return 0;
  SPR_REQUIRE(npairs <= 65535, "ransac_pairs: at most 65535 pairs per call (got %d)", npairs);
  SPR_REQUIRE(a && b && w && set_cu, "ransac_pairs: a, b, w and set_cu must not be null");
  SPR_REQUIRE(idx || pair_key, "ransac_pairs: pair_key (device) is needed when idx is null");
  SPR_REQUIRE(pose && best && score && hyp_pose && status, "ransac_pairs: null output pointer");
  const dim3 grid(cdiv(n_hyp, 4), npairs);
  if (idx)
    hipLaunchKernelGGL(k_ransac_hyp<false>, grid, dim3(256), 0, stream, a, b, w, set_cu, npairs, n_hyp, sample, seed,
                       pair_key, idx, score, hyp_pose);
  else
    hipLaunchKernelGGL(k_ransac_hyp<true>, grid, dim3(256), 0, stream, a, b, w, set_cu, npairs, n_hyp, sample, seed,
                       pair_key, idx, score, hyp_pose);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ransac_pick, dim3(npairs), dim3(64), 0, stream, set_cu, npairs, n_hyp, sample, idx, score,
                     hyp_pose, pose, best, status);
  SPR_LAUNCH_CHECK();
  return 0;
}
