// Raw KITTI scans of a whole batch -> the clouds the forward reads, in one call (include/spr.h, spr_prepare_scans).
//
// The loader (data_loaders/kitti_pred.py:203-230) runs, per scan: the first-point voxel filter, the radius crop, the
// ground cut -- the two masks on the FILTER's output, so a voxel whose first point is masked yields nothing.
//
//   1. k_ps_insert   one thread per point.  One int32 open-addressing table of 2n slots; cloud b owns the slots
//                    [2 cu[b], 2 cu[b+1]), so equal voxels of different clouds never meet and the cloud id is no part
//                    of the key.  A slot holds a point index + 1 (0 = empty), never a key: the key of a slot's owner is
//                    recomputed from its coordinates.  The first claim of a slot fixes its voxel for good (a slot only
//                    ever changes to another point of the SAME voxel, by atomicMin), so whatever the order of arrival
//                    every point of a voxel walks the same probe sequence to the same slot and the slot ends as the
//                    voxel's lowest index.  The table is touched by device-scope atomics only (the per-XCD L2s are not
//                    coherent: a plain load could see a stale line); the probe loop is bounded by the region's size.
//   2. k_ps_flag     one thread per slot: keep[owner] = mask predicate (float64, one rounding per operation).
//   3. k_ps_count    kept points per tile of kTile points.
//   4. k_ps_scan     one workgroup: exclusive scan of the tile counts, out_cu, status.
//   5. k_ps_compact  ordered write of out_xyz / out_idx.
//
// No sort, no library call; one memset clears table, flags, counts and the error bits together.
#include "spr_common.h"

namespace spr {
namespace {

constexpr int kTile = 1024;                 // points per workgroup of k_ps_count / k_ps_compact: 4 per thread
constexpr int kErrRange = 1, kErrProbe = 2, kErrLayout = 4;   // bits of the error word

struct PrepWs {
  int* err;              // [1] error bits (a 256-byte line of its own)
  int* table;            // [2n] point index + 1, 0 = empty
  int* tile;             // [ntile + 1] kept points per tile, then their exclusive prefix; [ntile] = m
  unsigned char* keep;   // [ntile * kTile] one byte per point (whole tiles: the tail reads as zeros)
};
size_t prep_tiles(int n) { return ((size_t)(n > 0 ? n : 1) + kTile - 1) / kTile; }
PrepWs prep_layout(Workspace& w, int n, int nb) {
  (void)nb;   // no part of the layout depends on the number of clouds
  const size_t N = (size_t)(n > 0 ? n : 1);
  PrepWs l;
  l.err = w.take<int>(1);
  l.table = w.take<int>(2 * N);
  l.tile = w.take<int>(prep_tiles(n) + 1);
  l.keep = w.take<unsigned char>(prep_tiles(n) * kTile);
  return l;
}

// 63-bit voxel key of a point: k_vox_keys' arithmetic (grid_subsample.hip).  false: a coordinate is not finite or lies
// outside +-2^20 voxels (tested before the conversion: converting NaN to an integer is undefined).
__device__ __forceinline__ bool voxel_key(const float* __restrict__ p, double voxel, unsigned long long& key) {
  unsigned long long k = 0;
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double q = (double)p[d] / voxel;   // Eigen: (point / voxel_size).cast<int>()
    if (!(fabs(q) < 1048576.0)) {
      ok = false;
      continue;
    }
    const long long c = (long long)q;        // truncation toward zero
    k = (k << 21) | (unsigned long long)((c + (1ll << 20)) & 0x1fffff);
  }
  key = k;
  return ok;
}

__device__ __forceinline__ unsigned int mix_key(unsigned long long k) {   // splitmix64 finaliser, upper half
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return (unsigned int)(k >> 32);
}

__global__ __launch_bounds__(256) void k_ps_insert(const float* __restrict__ pts, int stride,
                                                   const int* __restrict__ cu, int n, int nb, double voxel, int* table,
                                                   int* err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int b = find_segment(cu, nb, i);
  const int beg = cu[b], end = cu[b + 1];
  if (!(beg >= 0 && beg <= i && i < end && end <= n)) {   // cu is not a prefix over n points: touch nothing
    atomicOr(err, kErrLayout);
    return;
  }
  unsigned long long key;
  if (!voxel_key(pts + (size_t)i * stride, voxel, key)) {
    atomicOr(err, kErrRange);
    return;
  }
  const unsigned int slots = 2u * (unsigned int)(end - beg);            // < 2^32
  int* region = table + 2 * (size_t)beg;
  unsigned int s = (unsigned int)(((unsigned long long)mix_key(key) * slots) >> 32);   // < slots
  for (unsigned int probe = 0; probe < slots; ++probe) {
    const int old = atomicCAS(region + s, 0, i + 1);
    if (old == 0) return;                                                // first of its voxel so far
    unsigned long long other;
    voxel_key(pts + (size_t)(old - 1) * stride, voxel, other);           // owners passed the range test
    if (other == key) {
      if (i + 1 < old) atomicMin(region + s, i + 1);                     // the slot only ever falls: old already wins
      return;
    }
    if (++s == slots) s = 0;                                             // wrap inside the cloud's region
  }
  atomicOr(err, kErrProbe);   // every slot of the region belongs to another voxel: cannot happen at load <= 1/2
}

// The loader's two masks on a kept point, in float64 like its numpy lines: sqrt(x*x + y*y) <= crop_radius with one
// rounding per operation (a contracted x*x + y*y can land on the other side of the radius), z > -1 strictly.
__device__ __forceinline__ bool scan_mask(const float* __restrict__ p, double crop_radius, int remove_ground) {
  bool keep = true;
  if (crop_radius > 0.0) {
    const double x = (double)p[0], y = (double)p[1];
    const double r = __dsqrt_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)));
    keep = r <= crop_radius;
  }
  if (remove_ground) keep = keep && (double)p[2] > -1.0;
  return keep;
}

__global__ __launch_bounds__(256) void k_ps_flag(const float* __restrict__ pts, int stride,
                                                 const int* __restrict__ table, int n, double crop_radius,
                                                 int remove_ground, unsigned char* __restrict__ keep) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= 2 * (size_t)n) return;
  const int v = table[s];
  if (v <= 0 || v > n) return;
  if (scan_mask(pts + (size_t)(v - 1) * stride, crop_radius, remove_ground)) keep[v - 1] = 1;
}

// The four flags of thread t of a tile as one word; bytes beyond n are zero (memset, never written).
__device__ __forceinline__ unsigned int tile_flags(const unsigned char* __restrict__ keep, int tile) {
  return *(const unsigned int*)(keep + (size_t)tile * kTile + 4 * threadIdx.x);
}

// Sum of v over the 256 threads (every thread gets it) and the exclusive prefix of this thread.  sh: 4 ints.
__device__ __forceinline__ int block_scan_256(int v, int* sh, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += sh[w];
    total += sh[w];
  }
  __syncthreads();
  return before + inc - v;
}

__global__ __launch_bounds__(256) void k_ps_count(const unsigned char* __restrict__ keep, int* __restrict__ tile) {
  __shared__ int sh[4];
  int total;
  block_scan_256(__popc(tile_flags(keep, blockIdx.x)), sh, total);
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_ps_scan(int* tile, int ntile, const unsigned char* __restrict__ keep,
                                                          const int* __restrict__ cu, int n, int nb,
                                                          const int* __restrict__ err, int* __restrict__ out_cu,
                                                          int* __restrict__ status) {
  __shared__ int sh[kScanThreads];
  const int t = threadIdx.x;
  const int per = (ntile + kScanThreads - 1) / kScanThreads;
  const int lo = min(t * per, ntile), hi = min(lo + per, ntile);
  int sum = 0;
  for (int k = lo; k < hi; ++k) sum += tile[k];
  sh[t] = sum;
  __syncthreads();
  for (int o = 1; o < kScanThreads; o <<= 1) {   // inclusive scan of the threads' sums
    const int add = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  int run = sh[t] - sum;
  for (int k = lo; k < hi; ++k) {
    const int c = tile[k];
    tile[k] = run;
    run += c;
  }
  if (t == kScanThreads - 1) tile[ntile] = sh[t];   // m
  __threadfence_block();
  __syncthreads();
  // out_cu[b] = kept points in front of cu[b]: the prefix of its tile plus the flags of the tile up to it
  for (int b = t; b <= nb; b += kScanThreads) {
    const int pos = min(max(cu[b], 0), n);
    const int k = pos / kTile;   // == ntile only for pos == n on a tile boundary: nothing to add
    int c = tile[k];
    for (int j = k * kTile; j < pos; ++j) c += keep[j];
    out_cu[b] = c;
  }
  if (t == 0) {
    const int e = err[0];
    status[0] = (e & kErrLayout) ? SPR_PREPARE_BAD_LAYOUT : (e & kErrRange) ? SPR_PREPARE_RANGE
                : (e & kErrProbe) ? SPR_PREPARE_PROBE : 0;
  }
}

__global__ __launch_bounds__(256) void k_ps_compact(const float* __restrict__ pts, int stride,
                                                    const int* __restrict__ cu, int n, int nb,
                                                    const unsigned char* __restrict__ keep,
                                                    const int* __restrict__ tile, float* __restrict__ out_xyz,
                                                    int* __restrict__ out_idx) {
  __shared__ int sh[4];
  const unsigned int flags = tile_flags(keep, blockIdx.x);
  int total;
  int o = tile[blockIdx.x] + block_scan_256(__popc(flags), sh, total);
  if (flags == 0) return;
  const int first = blockIdx.x * kTile + 4 * threadIdx.x;   // < n + kTile: no overflow for n <= 2^31 - 1 - kTile
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = first + j;
    if (!((flags >> (8 * j)) & 0xff) || i >= n || o >= n) continue;
    const float* p = pts + (size_t)i * stride;
    out_xyz[3 * (size_t)o + 0] = p[0];
    out_xyz[3 * (size_t)o + 1] = p[1];
    out_xyz[3 * (size_t)o + 2] = p[2];
    out_idx[o] = i - cu[find_segment(cu, nb, i)];
    ++o;
  }
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_prepare_scans_scratch_len(int n, int nb) { return measure(prep_layout, n, nb) / sizeof(int); }

extern "C" int spr_prepare_scans(const float* pts, int stride, const int* cu, int n, int nb, double voxel_size,
                                 double crop_radius, int remove_ground, int* scratch, size_t scratch_len,
                                 float* out_xyz, int* out_idx, int* out_cu, int* status, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(pts && cu && scratch && out_xyz && out_idx && out_cu && status, "prepare_scans: null pointer");
  SPR_REQUIRE(stride == 3 || stride == 4, "prepare_scans: stride %d, must be 3 or 4", stride);
  SPR_REQUIRE(voxel_size > 0.0, "prepare_scans: voxel_size %g must be positive", voxel_size);   // false for NaN too
  SPR_REQUIRE(n >= 1 && nb >= 1, "prepare_scans: n %d and nb %d must be at least 1", n, nb);
  SPR_REQUIRE(nb <= n, "prepare_scans: %d clouds over %d points (every cloud holds at least one)", nb, n);
  SPR_REQUIRE(n <= INT32_MAX - kTile, "prepare_scans: n %d exceeds %d", n, INT32_MAX - kTile);
  SPR_REQUIRE(scratch_len <= SIZE_MAX / sizeof(int), "prepare_scans: scratch_len overflows");
  Workspace w(scratch, scratch_len * sizeof(int));
  const auto [err, table, tile, keep] = prep_layout(w, n, nb);
  SPR_REQUIRE(w.ok(), "prepare_scans: scratch too small (%zu ints, spr_prepare_scans_scratch_len gives %zu)",
              scratch_len, spr_prepare_scans_scratch_len(n, nb));
  const int ntile = (int)prep_tiles(n);
  SPR_HIP_CHECK(hipMemsetAsync(scratch, 0, w.used(), stream));
  hipLaunchKernelGGL(k_ps_insert, dim3(cdiv(n, 256)), dim3(256), 0, stream, pts, stride, cu, n, nb, voxel_size, table,
                     err);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ps_flag, dim3(cdiv(2 * (long)n, 256)), dim3(256), 0, stream, pts, stride, table, n, crop_radius,
                     remove_ground, keep);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ps_count, dim3(ntile), dim3(256), 0, stream, keep, tile);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ps_scan, dim3(1), dim3(kScanThreads), 0, stream, tile, ntile, keep, cu, n, nb, err, out_cu,
                     status);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ps_compact, dim3(ntile), dim3(256), 0, stream, pts, stride, cu, n, nb, keep, tile, out_xyz,
                     out_idx);
  SPR_LAUNCH_CHECK();
  return 0;
}
