// Training over shared clouds: what the pair assembly (pair_gather.hip) needs beside it when a cloud is encoded once and
// used by several pairs of a training step.
//
//   spr_pair_gather_bwd     the backward of spr_pair_gather: a cloud's row gradient is the sum over every output segment
//                           that copied it.  The grid is over INPUT rows; the segments of a cloud come from a use list
//                           in CSR form (use_ptr / use_seg, ascending segment index, built on the host) and are added
//                           in that stored order in registers, so the sum has one fixed order whatever the launch
//                           geometry: no atomics, every row of gx written exactly once (unused clouds: zeros).
//   spr_overlap_pool_pairs  one level of compute_overlaps (k_overlap_pool, losses.hip) for labels in pair layout over a
//                           pool matrix in cloud layout: the same arithmetic, the indices rebased per segment.
//
// Both are memory-bound walks in k_pair_gather's idiom: a wave owns a contiguous row range, finds where its first row
// lies by ONE wave-uniform binary search and then only walks forward; 16 bytes per lane where width and alignment allow,
// 4 bytes otherwise; the loads of a step are issued before its first store.  No LDS, plain vector stores.
#include "spr_common.h"

namespace spr {
namespace {

constexpr int kUnroll = 4;        // row groups in flight per wave step
constexpr int kWavesPerBlock = 4;
constexpr int kMaxBlocks = 2048;  // memory-bound: a capped grid, every wave walks a chunk of rows

__device__ __forceinline__ void clear(float& v) { v = 0.f; }
__device__ __forceinline__ void clear(float4& v) { v.x = v.y = v.z = v.w = 0.f; }
__device__ __forceinline__ void add(float& a, const float& b) { a += b; }
__device__ __forceinline__ void add(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// V: float4 (rows of w = C / 4 vectors, gy and gx 16-byte aligned) or float (w = C).
template <typename V>
__global__ __launch_bounds__(kWavesPerBlock* kWave) void k_pair_gather_bwd(
    const V* __restrict__ gy, int t_out, int w, const int* __restrict__ cu, int n_clouds,
    const int* __restrict__ use_ptr, const int* __restrict__ use_seg, int npairs, const int* __restrict__ cu_out,
    int t_in, int rows_per_wave, V* __restrict__ gx) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
  const long row_beg = (long)wave * rows_per_wave;
  if (row_beg >= t_in) return;
  const int row_end = (int)(row_beg + rows_per_wave < (long)t_in ? row_beg + rows_per_wave : (long)t_in);
  const int nseg = 2 * npairs;

  // lane -> (row of the group, first vector of the row); lanes behind the last whole row of a group idle
  const int group = w >= kWave ? 1 : kWave / w;   // rows per access
  const int r = w >= kWave ? 0 : lane / w;
  const int j0 = w >= kWave ? lane : lane - r * w;
  if (r >= group) return;

  int cloud = find_segment(cu, n_clouds, (int)row_beg);   // uniform
  int c_beg = 0, c_end = 0, u_beg = 0, u_end = 0;
  auto enter = [&](int c) {                               // the registers that describe cloud c
    c_beg = cu[c];
    c_end = cu[c + 1];
    u_beg = use_ptr[c] > 0 ? use_ptr[c] : 0;              // a malformed list never indexes outside use_seg
    u_end = use_ptr[c + 1] < nseg ? use_ptr[c + 1] : nseg;
  };
  enter(cloud);

  for (int base = (int)row_beg; base < row_end; base += group * kUnroll) {
    int local[kUnroll], first[kUnroll], uses[kUnroll];   // row inside its cloud, its first use, its number of uses
    int most = 0;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int row = base + u * group + r;
      local[u] = first[u] = uses[u] = 0;
      if (row < row_end) {
        while (row >= c_end && cloud + 1 < n_clouds) enter(++cloud);
        if (row >= c_beg && row < c_end && u_end > u_beg) {   // rows behind the last cloud belong to none: zeros
          local[u] = row - c_beg;
          first[u] = u_beg;
          uses[u] = u_end - u_beg;
        }
      }
      most = uses[u] > most ? uses[u] : most;
    }
    for (int j = j0; j < w; j += kWave) {
      V acc[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) clear(acc[u]);
      for (int k = 0; k < most; ++k) {                    // the k-th use of every row of the step: loads, then adds
        V v[kUnroll];
        int from[kUnroll];                                // the row of gy; -1: this use contributes zeros
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          from[u] = -1;
          if (k < uses[u]) {
            const int s = use_seg[first[u] + k];
            if ((unsigned)s < (unsigned)nseg) {           // a segment index out of range contributes nothing
              const int o_beg = cu_out[s];
              const long o_row = (long)o_beg + local[u];
              // a segment shorter than its cloud (cu_out does not describe the clouds): zeros for the rows it lacks
              if (o_beg >= 0 && o_row < cu_out[s + 1] && o_row < t_out) from[u] = (int)o_row;
            }
          }
          v[u] = gy[(size_t)(from[u] < 0 ? 0 : from[u]) * w + j];   // row 0 is always readable
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (from[u] < 0) clear(v[u]);
          if (k == 0)
            acc[u] = v[u];                                // the first use as it is (a lone use is a copy, -0 included)
          else if (k < uses[u])                           // nothing behind a row's last use, not even + 0 (-0 stays -0)
            add(acc[u], v[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int row = base + u * group + r;
        if (row < row_end) gx[(size_t)row * w + j] = acc[u];
      }
    }
  }
}

// One lane per output row.  rows_per_wave is a multiple of 64; the wave's first row gives the segment its lanes start
// from.  VEC: pool rows are read four columns at a time (stride % 4 == 0, 16-byte aligned base).
template <bool VEC>
__global__ __launch_bounds__(kWavesPerBlock* kWave) void k_overlap_pool_pairs(
    const float* __restrict__ ov, int n_prev, const int* __restrict__ pool, int stride, int w, int n_pool_rows,
    const int* __restrict__ cu_prev, const int* __restrict__ cu_cur, int n_clouds, const int* __restrict__ seg_cloud,
    int npairs, const int* __restrict__ cu_out_prev, const int* __restrict__ cu_out_cur, int nq, int rows_per_wave,
    float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
  const long row_beg = (long)wave * rows_per_wave;
  if (row_beg >= nq) return;
  const int row_end = (int)(row_beg + rows_per_wave < (long)nq ? row_beg + rows_per_wave : (long)nq);
  const int nseg = 2 * npairs;

  int seg = find_segment(cu_out_cur, nseg, (int)row_beg);   // uniform
  int seg_beg = 0, seg_end = 0;
  long prow0 = 0;         // pool row of the segment's first row; -1: the segment has none
  int prow_end = 0;       // end of the cloud's pool rows
  int lo = 0, hi = 0;     // the cloud's rows on the previous level: the ids that count
  long ov0 = 0;           // where the segment's labels of the previous level start
  int ov_len = 0;
  auto enter = [&](int s) {
    seg_beg = cu_out_cur[s];
    seg_end = cu_out_cur[s + 1];
    const int c = seg_cloud[s];
    prow0 = -1;
    prow_end = lo = hi = ov_len = 0;
    ov0 = 0;
    if ((unsigned)c < (unsigned)n_clouds) {
      prow0 = cu_cur[c];
      prow_end = cu_cur[c + 1] < n_pool_rows ? cu_cur[c + 1] : n_pool_rows;
      lo = cu_prev[c];
      hi = cu_prev[c + 1];
      ov0 = cu_out_prev[s];
      const long room = (long)n_prev - ov0;                 // labels that exist behind ov0
      const long len = (long)cu_out_prev[s + 1] - ov0;
      ov_len = (int)(len < room ? len : room);
      if (ov0 < 0 || prow0 < 0 || lo < 0) prow0 = -1;     // prefixes that are none: the segment reads nothing
    }
  };
  enter(seg);

  for (int row = (int)row_beg + lane; row < row_end; row += kWave) {
    while (row >= seg_end && seg + 1 < nseg) enter(++seg);
    const long prow = prow0 + (row - seg_beg);
    float s = 0.f;
    int cnt = 0;
    // a row without a pool row of its own cloud has no valid entry: 0 / 0, like a row of shadow entries only
    if (row >= seg_beg && row < seg_end && prow0 >= 0 && prow < prow_end) {
      const int* __restrict__ p = pool + (size_t)prow * stride;
      auto take = [&](int id, float v) {                    // ascending columns, k_overlap_pool's order
        if (id >= lo && id < hi && id - lo < ov_len) {
          s += v;
          ++cnt;
        }
      };
      auto fetch = [&](int id) {                            // entries that do not count read label 0 (always there)
        return ov[id >= lo && id < hi && id - lo < ov_len ? (size_t)(ov0 + (id - lo)) : (size_t)0];
      };
      int k = 0;
      if (VEC) {
        for (; k + 8 <= w; k += 8) {                        // two 16-byte index loads, then their eight labels
          const int4 a = *(const int4*)(p + k), b = *(const int4*)(p + k + 4);
          const float v0 = fetch(a.x), v1 = fetch(a.y), v2 = fetch(a.z), v3 = fetch(a.w);
          const float v4 = fetch(b.x), v5 = fetch(b.y), v6 = fetch(b.z), v7 = fetch(b.w);
          take(a.x, v0), take(a.y, v1), take(a.z, v2), take(a.w, v3);
          take(b.x, v4), take(b.y, v5), take(b.z, v6), take(b.w, v7);
        }
        for (; k + 4 <= w; k += 4) {
          const int4 a = *(const int4*)(p + k);
          const float v0 = fetch(a.x), v1 = fetch(a.y), v2 = fetch(a.z), v3 = fetch(a.w);
          take(a.x, v0), take(a.y, v1), take(a.z, v2), take(a.w, v3);
        }
      } else {
        for (; k + 4 <= w; k += 4) {
          const int i0 = p[k], i1 = p[k + 1], i2 = p[k + 2], i3 = p[k + 3];
          const float v0 = fetch(i0), v1 = fetch(i1), v2 = fetch(i2), v3 = fetch(i3);
          take(i0, v0), take(i1, v1), take(i2, v2), take(i3, v3);
        }
      }
      for (; k < w; ++k) {
        const int id = p[k];
        take(id, fetch(id));
      }
    }
    const float v = s / (float)cnt;
    out[row] = v != v ? v : fminf(fmaxf(v, 0.f), 1.f);
  }
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" int spr_pair_gather_bwd(const float* gy, int t_out, int c, const int* cu, int n_clouds, const int* use_ptr,
                                   const int* use_seg, int npairs, const int* cu_out, int t_in, float* gx,
                                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(gy != nullptr && gx != nullptr && cu != nullptr && use_ptr != nullptr && use_seg != nullptr &&
                  cu_out != nullptr,
              "pair_gather_bwd: null pointer");
  SPR_REQUIRE(t_in > 0 && t_out > 0 && c >= 1 && n_clouds >= 1 && npairs >= 1 && npairs <= (1 << 29) &&
                  t_out <= (1 << 30) && t_in <= (1 << 30),
              "pair_gather_bwd: bad arguments (t_in %d, t_out %d, c %d, clouds %d, pairs %d)", t_in, t_out, c,
              n_clouds, npairs);
  const bool vec = c % 4 == 0 && (((uintptr_t)gy | (uintptr_t)gx) & 15) == 0;
  const int w = vec ? c / 4 : c;
  const int step = (w >= kWave ? 1 : kWave / w) * kUnroll;       // rows one wave sums per step
  const long steps = ((long)t_in + step - 1) / step;
  long nwaves = steps < (long)kMaxBlocks * kWavesPerBlock ? steps : (long)kMaxBlocks * kWavesPerBlock;
  const long per_wave = (steps + nwaves - 1) / nwaves * step;    // a multiple of `step`: groups never straddle two waves
  nwaves = ((long)t_in + per_wave - 1) / per_wave;
  const unsigned grid = (unsigned)((nwaves + kWavesPerBlock - 1) / kWavesPerBlock);
  if (vec)
    hipLaunchKernelGGL(k_pair_gather_bwd<float4>, dim3(grid), dim3(kWavesPerBlock * kWave), 0, stream,
                       (const float4*)gy, t_out, w, cu, n_clouds, use_ptr, use_seg, npairs, cu_out, t_in,
                       (int)per_wave, (float4*)gx);
  else
    hipLaunchKernelGGL(k_pair_gather_bwd<float>, dim3(grid), dim3(kWavesPerBlock * kWave), 0, stream, gy, t_out, w, cu,
                       n_clouds, use_ptr, use_seg, npairs, cu_out, t_in, (int)per_wave, gx);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_overlap_pool_pairs(const float* ov_prev, int n_prev, const int* pool, int pool_stride, int w,
                                      int n_pool_rows, const int* cu_prev, const int* cu_cur, int n_clouds,
                                      const int* seg_cloud, int npairs, const int* cu_out_prev, const int* cu_out_cur,
                                      int nq, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(ov_prev != nullptr && pool != nullptr && cu_prev != nullptr && cu_cur != nullptr &&
                  seg_cloud != nullptr && cu_out_prev != nullptr && cu_out_cur != nullptr && out != nullptr,
              "overlap_pool_pairs: null pointer");
  SPR_REQUIRE(nq >= 1 && nq <= (1 << 30) && w >= 1 && pool_stride >= w && n_prev >= 1 && n_pool_rows >= 1 &&
                  n_clouds >= 1 && npairs >= 1 && npairs <= (1 << 29),
              "overlap_pool_pairs: bad sizes (rows %d, width %d, stride %d, labels %d, pool rows %d, clouds %d, pairs %d)",
              nq, w, pool_stride, n_prev, n_pool_rows, n_clouds, npairs);
  const bool vec = pool_stride % 4 == 0 && ((uintptr_t)pool & 15) == 0;
  const long steps = ((long)nq + kWave - 1) / kWave;             // 64 rows per wave step
  long nwaves = steps < (long)kMaxBlocks * kWavesPerBlock ? steps : (long)kMaxBlocks * kWavesPerBlock;
  const long per_wave = (steps + nwaves - 1) / nwaves * kWave;
  nwaves = ((long)nq + per_wave - 1) / per_wave;
  const unsigned grid = (unsigned)((nwaves + kWavesPerBlock - 1) / kWavesPerBlock);
  if (vec)
    hipLaunchKernelGGL(k_overlap_pool_pairs<true>, dim3(grid), dim3(kWavesPerBlock * kWave), 0, stream, ov_prev, n_prev,
                       pool, pool_stride, w, n_pool_rows, cu_prev, cu_cur, n_clouds, seg_cloud, npairs, cu_out_prev,
                       cu_out_cur, nq, (int)per_wave, out);
  else
    hipLaunchKernelGGL(k_overlap_pool_pairs<false>, dim3(grid), dim3(kWavesPerBlock * kWave), 0, stream, ov_prev,
                       n_prev, pool, pool_stride, w, n_pool_rows, cu_prev, cu_cur, n_clouds, seg_cloud, npairs,
                       cu_out_prev, cu_out_cur, nq, (int)per_wave, out);
  SPR_LAUNCH_CHECK();
  return 0;
}
