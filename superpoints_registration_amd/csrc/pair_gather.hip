// Pair assembly: encoded clouds -> the [src_0..src_{P-1}, tgt_0..tgt_{P-1}] token layout (spr_pair_gather).
//
// A pure copy.  Output segment s is cloud src_idx[s] (s < P) or tgt_idx[s - P]; both the source cloud and the output
// segment are contiguous row ranges, so a row's source is row + (cu[cloud] - cu_out[s]).  Every wave owns a contiguous
// range of output rows: it finds the segment of its first row by ONE binary search in cu_out (wave-uniform: scalar
// loads) and then only walks forward, keeping the current segment's end and row offset in registers -- no per-row
// index tensor.  A step of a wave moves kUnroll groups of whole rows: at 16 bytes per lane a 1 KB token row
// (C = 256) is one coalesced 64-lane access, narrower rows share a wave (64 / width rows per access), wider rows take
// several.  All loads of a step are issued before its stores.  No atomics, plain vector stores.
#include "spr_common.h"

namespace spr {
namespace {

constexpr int kUnroll = 4;        // row groups in flight per wave step
constexpr int kWavesPerBlock = 4;
constexpr int kMaxBlocks = 2048;  // memory-bound: a capped grid, every wave walks a chunk of rows

__device__ __forceinline__ void clear(float& v) { v = 0.f; }
__device__ __forceinline__ void clear(float4& v) { v.x = v.y = v.z = v.w = 0.f; }

// V: float4 (rows of w = C / 4 vectors, x and y 16-byte aligned) or float (w = C).
template <typename V>
__global__ __launch_bounds__(kWavesPerBlock* kWave) void k_pair_gather(
    const V* __restrict__ x, int t_in, int w, const int* __restrict__ cu, int n_clouds, const int* __restrict__ src_idx,
    const int* __restrict__ tgt_idx, int npairs, const int* __restrict__ cu_out, int t_out, int rows_per_wave,
    V* __restrict__ y) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
  const long row_beg = (long)wave * rows_per_wave;
  if (row_beg >= t_out) return;
  const int row_end = (int)(row_beg + rows_per_wave < (long)t_out ? row_beg + rows_per_wave : (long)t_out);
  const int nseg = 2 * npairs;

  // lane -> (row of the group, first vector of the row); lanes behind the last whole row of a group idle
  const int group = w >= kWave ? 1 : kWave / w;   // rows per access
  const int r = w >= kWave ? 0 : lane / w;
  const int j0 = w >= kWave ? lane : lane - r * w;
  if (r >= group) return;

  int seg = find_segment(cu_out, nseg, (int)row_beg);   // uniform
  int seg_end = 0, src_end = 0;
  long delta = 0;
  auto enter = [&](int s) {                             // the registers that describe segment s
    seg_end = cu_out[s + 1];
    const int c = s < npairs ? src_idx[s] : tgt_idx[s - npairs];
    if ((unsigned)c < (unsigned)n_clouds) {
      delta = (long)cu[c] - cu_out[s];
      src_end = cu[c + 1] <= t_in ? cu[c + 1] : t_in;
    } else {                                            // bad index: the segment reads zeros
      delta = 0;
      src_end = 0;
    }
  };
  enter(seg);

  for (int base = (int)row_beg; base < row_end; base += group * kUnroll) {
    V v[kUnroll];
    size_t src[kUnroll];   // first vector of the source row; row 0 (always readable) + ok = false: zeros
    bool ok[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int row = base + u * group + r;
      src[u] = 0;
      ok[u] = false;
      if (row < row_end) {
        while (row >= seg_end && seg + 1 < nseg) enter(++seg);
        const long s_row = row + delta;
        // a source row outside its cloud (cu_out does not describe the indexed clouds) reads zeros
        if (row < seg_end && s_row >= 0 && s_row < src_end) {
          src[u] = (size_t)s_row * w;
          ok[u] = true;
        }
      }
    }
    for (int j = j0; j < w; j += kWave) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = x[src[u] + j];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int row = base + u * group + r;
        if (!ok[u]) clear(v[u]);
        if (row < row_end) y[(size_t)row * w + j] = v[u];
      }
    }
  }
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" int spr_pair_gather(const float* x, int t_in, int c, const int* cu, int n_clouds, const int* src_idx,
                               const int* tgt_idx, int npairs, const int* cu_out, int t_out, float* y, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(x != nullptr && y != nullptr && cu != nullptr && src_idx != nullptr && tgt_idx != nullptr &&
                  cu_out != nullptr,
              "pair_gather: null pointer");
  SPR_REQUIRE(t_in > 0 && t_out > 0 && c >= 1 && n_clouds >= 1 && npairs >= 1 && npairs <= (1 << 29) &&
                  t_out <= (1 << 30),
              "pair_gather: bad arguments (t_in %d, t_out %d, c %d, clouds %d, pairs %d)", t_in, t_out, c, n_clouds,
              npairs);
  const bool vec = c % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  const int w = vec ? c / 4 : c;
  const int step = (w >= kWave ? 1 : kWave / w) * kUnroll;       // rows one wave moves per step
  const long steps = ((long)t_out + step - 1) / step;
  long nwaves = steps < (long)kMaxBlocks * kWavesPerBlock ? steps : (long)kMaxBlocks * kWavesPerBlock;
  const long per_wave = (steps + nwaves - 1) / nwaves * step;    // a multiple of `step`: groups never straddle two waves
  nwaves = ((long)t_out + per_wave - 1) / per_wave;
  const unsigned grid = (unsigned)((nwaves + kWavesPerBlock - 1) / kWavesPerBlock);
  if (vec)
    hipLaunchKernelGGL(k_pair_gather<float4>, dim3(grid), dim3(kWavesPerBlock * kWave), 0, stream,
                       (const float4*)x, t_in, w, cu, n_clouds, src_idx, tgt_idx, npairs, cu_out, t_out, (int)per_wave,
                       (float4*)y);
  else
    hipLaunchKernelGGL(k_pair_gather<float>, dim3(grid), dim3(kWavesPerBlock * kWave), 0, stream, x, t_in, w, cu,
                       n_clouds, src_idx, tgt_idx, npairs, cu_out, t_out, (int)per_wave, y);
  SPR_LAUNCH_CHECK();
  return 0;
}
