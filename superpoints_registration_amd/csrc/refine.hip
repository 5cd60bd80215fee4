// The config-off refinements of RegTR.softmax_correlation for ALL pairs of a batch in one launch (spr_refine_pairs;
// qk_regtr_full.py:370-398, :455-556, :563-658; contract in include/spr.h).
//
// One 256-thread workgroup per pair; nothing crosses pairs, there are no atomics and every reduction has a fixed order,
// so a pair gives the same bits alone or anywhere in any batch.  Per pair:
//   v[i]          the own side's match values (the tgt tokens when N > M, else the src tokens), ratio test applied
//   median        exact: the entries are sorted as 64-bit keys (order-preserving value bits | ~index) by a bitonic
//                 network and the element at ascending position (n-1)/2 is read off
//   overlap       ov = ov_s * ov_t over (entry, partner); v *= ov unless the overlap is the Procrustes weight
//   top-k         the same sort on the final values: descending, ties to the lower index; first k_b entries
//   gather        val / ind / both point sets in that order to the packed outputs
//   pose          procrustes_block (the solve of spr_weighted_procrustes, same order of operations) on the gathered
//                 points, read back from the outputs this workgroup has just written
//   LGR           n_steps x (residuals in spr_pose_residuals' arithmetic, w *= res < radius, re-solve)
// Working set: keys [P] u64 (P = n rounded up to a power of two), v [n], solve weights [k], LGR weights [k].  For
// n <= kLdsN = 4096 that is 80 KiB of the CU's 160 KiB LDS (dynamic); a pair with more entries, up to
// SPR_REFINE_MAX_N, keeps the same four arrays in the caller's workspace (L2 resident: 20 bytes per entry).
#include "procrustes_solve.h"
#include "spr_common.h"

namespace spr {
namespace {

constexpr int kThreads = 256;
constexpr int kLdsN = 4096;   // entries per pair whose working set stays in LDS
constexpr size_t kLdsBytes = (size_t)kLdsN * (8 + 4 + 4 + 4);

__host__ __device__ inline int pow2_ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
__host__ __device__ inline size_t align_up_c(size_t x) { return (x + 255) / 256 * 256; }
// bytes of one pair's working set for up to n entries (keys, v, w1, wl), every array 256-byte aligned
__host__ __device__ inline size_t pair_bytes(int n) { return (size_t)pow2_ceil(n) * 8 + 3 * align_up_c((size_t)n * 4); }

// float -> u32 whose unsigned order is the float order (-0 < +0; NaNs at the ends)
__device__ __forceinline__ unsigned int ord_bits(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// keys[0..P) descending; every thread of the workgroup calls this, barriers inside and one behind
__device__ void bitonic_desc(unsigned long long* keys, int P) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (P >> 1); t += kThreads) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const unsigned long long x = keys[i], y = keys[j];
        const bool desc = (i & size) == 0;
        if (desc ? (x < y) : (x > y)) {
          keys[i] = y;
          keys[j] = x;
        }
      }
    }
  __syncthreads();
}

// keys of v[0..n): value bits above the inverted index, so that a descending sort puts the lower index first among
// equal values; padding (0) sorts behind every entry
__device__ void build_keys(unsigned long long* keys, const float* v, int n, int P) {
  for (int i = threadIdx.x; i < P; i += kThreads)
    keys[i] = i < n ? ((unsigned long long)ord_bits(v[i]) << 32) | (unsigned int)(~(unsigned int)i) : 0ull;
}

__global__ __launch_bounds__(kThreads) void k_refine_pairs(
    const float* __restrict__ val, const float* __restrict__ val2, const int* __restrict__ ind,
    const float* __restrict__ overlap, const float* __restrict__ xyz, const int* __restrict__ cu, int npairs, int t_total,
    const int* __restrict__ k_b, const int* __restrict__ out_cu, int flags, float lowe_thres, float radius, int n_steps,
    const float* __restrict__ pose_in, int max_n, float* __restrict__ pose, float* __restrict__ val_out,
    long long* __restrict__ ind_out, float* __restrict__ src_pts, float* __restrict__ tgt_pts, int* __restrict__ status,
    char* __restrict__ ws, size_t ws_pair) {
  extern __shared__ __align__(16) char lds[];
  __shared__ double sh[256];
  __shared__ float s_pose[12];
  __shared__ int s_bad;

  const int b = blockIdx.x;
  const int s0 = cu[b], s1 = cu[b + 1], t0 = cu[npairs + b], t1 = cu[npairs + b + 1];
  const int N = s1 - s0, M = t1 - t0;
  const bool on_tgt = N > M;
  const int n = on_tgt ? M : N;
  const int own0 = on_tgt ? t0 : s0;
  const int plen = on_tgt ? N : M;          // length of the partner cloud: the range of ind
  const int k = k_b[b], o0 = out_cu[b];
  float* po = pose + 12 * (size_t)b;

  // structural errors: nothing of this pair is read or written beyond its pose (zeros) and status
  const bool bad_layout = s0 < 0 || N < 0 || M < 0 || t0 < s1 || t1 > t_total || n > max_n || k < 0 || k > n ||
                          o0 < 0 || out_cu[b + 1] - o0 != k;
  if (bad_layout) {
    if (threadIdx.x < 12) po[threadIdx.x] = 0.f;
    if (threadIdx.x == 0) status[b] = SPR_REFINE_BAD_LAYOUT;
    return;
  }
  if (threadIdx.x == 0) s_bad = 0;

  const int P = pow2_ceil(n);
  char* base = n <= kLdsN ? lds : ws + (size_t)b * ws_pair;
  const int cap = n <= kLdsN ? kLdsN : max_n;
  unsigned long long* keys = (unsigned long long*)base;
  float* v = (float*)(base + (size_t)pow2_ceil(cap) * 8);
  float* w1 = (float*)((char*)v + align_up_c((size_t)cap * 4));
  float* wl = (float*)((char*)w1 + align_up_c((size_t)cap * 4));

  const bool f_ratio = flags & SPR_REFINE_RATIO, f_median = flags & SPR_REFINE_MEDIAN;
  const bool f_ov = flags & SPR_REFINE_OVERLAP, f_ovw = flags & SPR_REFINE_OVERLAP_W;
  const bool f_topk = flags & SPR_REFINE_TOPK, f_lgr = flags & SPR_REFINE_LGR, f_sink = flags & SPR_REFINE_SINKHORN;

  // 1-2. own-side values, Lowe ratio test (0/0 = NaN fails it, like torch.where)
  for (int i = threadIdx.x; i < n; i += kThreads) {
    float x = val[own0 + i];
    if (f_ratio) x = (__fdiv_rn(val2[own0 + i], x) < lowe_thres) ? x : 0.f;
    v[i] = x;
  }
  __syncthreads();

  // 3. median threshold: torch's lower median = ascending position (n-1)/2 = descending position n-1-(n-1)/2
  if (f_median && n > 0) {
    build_keys(keys, v, n, P);
    bitonic_desc(keys, P);
    const float med = v[~(unsigned int)keys[n - 1 - (n - 1) / 2]];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kThreads) v[i] = v[i] > med ? v[i] : 0.f;
    __syncthreads();
  }

  // 4. overlap of (entry, partner); an index outside the partner cloud is reported and read as partner 0
  auto partner = [&](int i) {
    const int j = ind[own0 + i];
    if ((unsigned)j >= (unsigned)plen) {
      s_bad = 1;
      return 0;
    }
    return j;
  };
  auto ov_of = [&](int i, int j) {
    return on_tgt ? overlap[s0 + j] * overlap[t0 + i] : overlap[s0 + i] * overlap[t0 + j];
  };
  if (f_ov && !f_ovw) {
    for (int i = threadIdx.x; i < n; i += kThreads) v[i] = v[i] * ov_of(i, partner(i));
    __syncthreads();
  }

  // 5. top-k order
  if (f_topk && n > 0) {
    build_keys(keys, v, n, P);
    bitonic_desc(keys, P);
  }

  // gather by that order: packed outputs, solve weights w1, LGR weights wl
  for (int j = threadIdx.x; j < k; j += kThreads) {
    const int pos = f_topk ? (int)(~(unsigned int)keys[j]) : j;
    const int m = partner(pos);
    const float x = v[pos];
    val_out[o0 + j] = x;
    ind_out[o0 + j] = f_topk ? pos : m;     // after top-k the reference returns the top-k positions (:500, :611)
    const int ia = (f_sink || !on_tgt) ? s0 + pos : s0 + m;
    const int ib = (f_sink || on_tgt) ? t0 + pos : t0 + m;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      src_pts[3 * (size_t)(o0 + j) + d] = xyz[3 * (size_t)ia + d];
      tgt_pts[3 * (size_t)(o0 + j) + d] = xyz[3 * (size_t)ib + d];
    }
    w1[j] = f_ovw ? ov_of(pos, m) : x;
    wl[j] = x;
  }
  __threadfence_block();
  __syncthreads();

  const float* pa = src_pts + 3 * (size_t)o0;
  const float* pb = tgt_pts + 3 * (size_t)o0;
  auto fa = [&](int i, int d) { return pa[3 * (size_t)i + d]; };
  auto fb = [&](int i, int d) { return pb[3 * (size_t)i + d]; };

  // 6. pose of the surviving set, or the caller's (Sinkhorn) pose
  if (pose_in) {
    if (threadIdx.x < 12) s_pose[threadIdx.x] = pose_in[12 * (size_t)b + threadIdx.x];
  } else {
    procrustes_block(k, true, fa, fb, [&](int i) { return w1[i]; }, sh, s_pose);
  }
  __syncthreads();

  // 7. LGR (recompute_weights + compute_rigid_transform, :386-398)
  if (f_lgr)
    for (int step = 0; step < n_steps; ++step) {
      float T[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) T[q] = s_pose[q];
      for (int i = threadIdx.x; i < k; i += kThreads) {
        const float x = fa(i, 0), y = fa(i, 1), z = fa(i, 2);
        float d2 = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float e = fb(i, r) - ((x * T[4 * r] + y * T[4 * r + 1] + z * T[4 * r + 2]) + T[4 * r + 3]);
          d2 += e * e;
        }
        wl[i] = wl[i] * (sqrtf(d2) < radius ? 1.f : 0.f);
      }
      __syncthreads();          // every thread has read s_pose and written its weights
      procrustes_block(k, true, fa, fb, [&](int i) { return wl[i]; }, sh, s_pose);
      __syncthreads();
    }

  if (threadIdx.x < 12) po[threadIdx.x] = s_pose[threadIdx.x];
  if (threadIdx.x == 0) status[b] = s_bad ? SPR_REFINE_BAD_INDEX : 0;
}

}  // namespace
}  // namespace spr

using namespace spr;

// pairs too long for LDS: one working set per pair, which the kernel carves by pair_bytes as it carves LDS
static bool refine_needs_ws(int npairs, int max_n) { return npairs >= 1 && max_n > kLdsN && max_n <= SPR_REFINE_MAX_N; }
static char* refine_layout(Workspace& w, int npairs, int max_n) { return w.take<char>((size_t)npairs * pair_bytes(max_n)); }

extern "C" size_t spr_refine_pairs_workspace_bytes(int npairs, int max_n) {
  if (!refine_needs_ws(npairs, max_n)) return 0;
  return measure(refine_layout, npairs, max_n);
}

extern "C" int spr_refine_pairs(const float* val, const float* val2, const int* ind, const float* overlap,
                                const float* xyz, const int* cu, int npairs, int t_total, const int* k_b,
                                const int* out_cu, int flags, float lowe_thres, float acceptance_radius, int n_steps,
                                const float* pose_in, int max_n, float* pose, float* val_out, long long* ind_out,
                                float* src_pts, float* tgt_pts, int* status, void* ws, size_t ws_bytes,
                                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(val && ind && overlap && xyz && cu && k_b && out_cu && pose && val_out && ind_out && src_pts && tgt_pts &&
                  status,
              "refine_pairs: null pointer");
  SPR_REQUIRE(npairs >= 1 && t_total >= 0 && n_steps >= 0 && max_n >= 0, "refine_pairs: bad arguments (pairs %d, "
              "tokens %d, steps %d, max_n %d)", npairs, t_total, n_steps, max_n);
  SPR_REQUIRE((flags & ~SPR_REFINE_ALL_FLAGS) == 0, "refine_pairs: unknown flag bits 0x%x", flags);
  SPR_REQUIRE(!(flags & SPR_REFINE_RATIO) || val2, "refine_pairs: the ratio test needs val2");
  SPR_REQUIRE(!(flags & SPR_REFINE_OVERLAP_W) || (flags & SPR_REFINE_OVERLAP),
              "refine_pairs: overlap as weights needs the overlap switch");
  SPR_REQUIRE(!(flags & SPR_REFINE_SINKHORN) || pose_in, "refine_pairs: the Sinkhorn mode needs pose_in");
  SPR_REQUIRE(max_n <= SPR_REFINE_MAX_N, "refine_pairs: %d entries in one pair, the cap is %d", max_n,
              SPR_REFINE_MAX_N);
  const bool need = refine_needs_ws(npairs, max_n);
  Workspace w(ws, ws_bytes);
  char* sets = need ? refine_layout(w, npairs, max_n) : nullptr;
  SPR_REQUIRE(!need || (ws != nullptr && w.ok()), "refine_pairs: workspace of %zu bytes is too small", ws_bytes);
  if (int rc = ensure_dyn_lds((const void*)k_refine_pairs, (int)kLdsBytes)) return rc;
  hipLaunchKernelGGL(k_refine_pairs, dim3(npairs), dim3(kThreads), kLdsBytes, stream, val, val2, ind, overlap, xyz, cu,
                     npairs, t_total, k_b, out_cu, flags, lowe_thres, acceptance_radius, n_steps, pose_in, max_n, pose,
                     val_out, ind_out, src_pts, tgt_pts, status, sets, need ? pair_bytes(max_n) : (size_t)0);
  SPR_LAUNCH_CHECK();
  return 0;
}
