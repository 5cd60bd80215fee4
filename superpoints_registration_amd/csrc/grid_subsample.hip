// a1 -- batched voxel-grid barycentre subsampling on gfx950.
//
// Behaviour contract: batch_grid_subsampling()
//   /root/reference/src/models/backbone_kpconv/cpp_wrappers/cpp_subsampling/
//   grid_subsampling/grid_subsampling.cpp:5-106 (per cloud) and :109-204.
//
// MI355X design (not a translation of the hash-map loop):
//   1. one workgroup per cloud reduces the bounding box -> origin, nx, ny;
//   2. one thread per point builds a 64-bit key (cloud << 40 | voxel key);
//   3. rocPRIM radix sort of (key, point index) -- stable, so every voxel's
//      points stay in original order;
//   4. head flags + scan -> voxel ids; one thread per voxel sums its points
//      IN ORIGINAL ORDER in float32 and scales by (float)(1.0/count), which
//      reproduces the reference barycentre bit for bit;
//   5. output order: canonical (ascending key, spatially coherent -> better
//      gather locality downstream) or REFERENCE order.  The reference emits
//      voxels in libstdc++ std::unordered_map iteration order; that order is
//      re-derived on the GPU by replaying the hashtable's rehash epochs with
//      parallel passes (bucket-first-arrival atomics + scan), one workgroup
//      per cloud -- see k_umap_order.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <mutex>
#include <unordered_map>
#include <vector>

#include "spr_common.h"

namespace spr {
namespace {

constexpr int kKeyBits = 40;
constexpr unsigned long long kKeyMask = (1ull << kKeyBits) - 1;
// Bit 63 of a point / voxel key: the reference's 64-bit key is wrapped (see k_keys).  Above the cloud bits
// (nb < 2^23) and outside the bit range the radix sort looks at.
constexpr unsigned long long kKeyWrapped = 1ull << 63;
constexpr int kMaxSched = 40;

struct CloudInfo {
  float org[3];
  unsigned int nx, ny, nz;
};

// The bucket schedule travels as a kernel ARGUMENT (160 bytes): no per-device constant
// upload, no process-wide once-flag -- correct on whichever device the stream belongs to.
struct SchedArg {
  unsigned int v[kMaxSched];
};

// ---- bucket schedule of the platform's libstdc++ ---------------------------
// Measured, not assumed: drive a real std::unordered_map<size_t,char> and
// record every bucket_count() transition (same policy object the reference's
// std::unordered_map<size_t,SampledData> uses).
struct Schedule {
  std::vector<unsigned int> buckets;  // [0] = 1 (initial), then each growth
};
template <class Map>
std::vector<unsigned int> measure_schedule(size_t upto) {
  std::vector<unsigned int> out;
  Map m;
  size_t bc = m.bucket_count();
  out.push_back((unsigned int)bc);
  for (size_t i = 0; i < upto; ++i) {
    m.emplace((typename Map::key_type)i, 0);
    if (m.bucket_count() != bc) {
      bc = m.bucket_count();
      out.push_back((unsigned int)bc);
    }
  }
  return out;
}
const Schedule& host_schedule() {
  static Schedule s;
  static std::once_flag once;
  std::call_once(once, [] {
    s.buckets = measure_schedule<std::unordered_map<size_t, char>>((size_t)1 << 22);  // clouds up to 4M voxels
  });
  return s;
}
// The same measurement on the container of the label vote, std::unordered_map<int, int> (grid_subsampling.h:20), for
// voxels of up to `keys` distinct labels.  A voxel holds at most n labels, so the caller asks for n: measured once per
// power of two, the largest kept.
Schedule label_schedule(size_t keys) {
  static Schedule s;
  static size_t covered = 0;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (keys > covered) {
    size_t upto = (size_t)1 << 16;
    while (upto < keys) upto <<= 1;
    s.buckets = measure_schedule<std::unordered_map<int, int>>(upto);
    covered = upto;
  }
  return s;
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bbox(const float* __restrict__ xyz,
                                              const int* __restrict__ cu,
                                              float dl, CloudInfo* info) {
  const int c = blockIdx.x;
  const int beg = cu[c], end = cu[c + 1];
  __shared__ float smn[3][256], smx[3][256];
  float mn[3], mx[3];
  if (end > beg) {
    for (int d = 0; d < 3; ++d) mn[d] = mx[d] = xyz[3 * (size_t)beg + d];
  } else {
    for (int d = 0; d < 3; ++d) mn[d] = mx[d] = 0.f;
  }
  for (int i = beg + threadIdx.x; i < end; i += blockDim.x) {
    for (int d = 0; d < 3; ++d) {
      float v = xyz[3 * (size_t)i + d];
      if (v < mn[d]) mn[d] = v;
      if (v > mx[d]) mx[d] = v;
    }
  }
  for (int d = 0; d < 3; ++d) {
    smn[d][threadIdx.x] = mn[d];
    smx[d][threadIdx.x] = mx[d];
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      for (int d = 0; d < 3; ++d) {
        float a = smn[d][threadIdx.x + s];
        if (a < smn[d][threadIdx.x]) smn[d][threadIdx.x] = a;
        float b = smx[d][threadIdx.x + s];
        if (b > smx[d][threadIdx.x]) smx[d][threadIdx.x] = b;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // grid_subsampling.cpp:27,30-31 -- float32, no contraction.
    const float inv = __fdiv_rn(1.0f, dl);
    CloudInfo ci;
    for (int d = 0; d < 3; ++d)
      ci.org[d] = __fmul_rn(floorf(__fmul_rn(smn[d][0], inv)), dl);
    ci.nx = (unsigned int)floorf(__fdiv_rn(__fsub_rn(smx[0][0], ci.org[0]), dl)) + 1u;
    ci.ny = (unsigned int)floorf(__fdiv_rn(__fsub_rn(smx[1][0], ci.org[1]), dl)) + 1u;
    ci.nz = (unsigned int)floorf(__fdiv_rn(__fsub_rn(smx[2][0], ci.org[2]), dl)) + 1u;  // only bounds the keys
    info[c] = ci;
  }
}

__global__ void k_keys(const float* __restrict__ xyz, const int* __restrict__ cu,
                       int n, int nb, float dl, const CloudInfo* __restrict__ info,
                       unsigned long long* keys, int* vals, int* err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = find_segment(cu, nb, i);
  const CloudInfo ci = info[c];
  // grid_subsampling.cpp:53-56.  The origin floor(min * (1/dl)) * dl can round to just ABOVE the cloud's minimum;
  // the cell index of a point below it is floor(tiny negative) = -1, and the reference's (size_t) cast of it is the
  // x86-64 one: 2^64 - 1, the key arithmetic wrapping modulo 2^64.  So the indices are signed here (the GPU's
  // float -> unsigned long long conversion of -1.0f gives 2^32 - 1) and the key is their sum modulo 2^64: a point with
  // ix = -1, iy >= 1 shares voxel (nx - 1, iy - 1); with iy = iz = 0 it has the key 2^64 - 1 and a voxel of its own.
  const long long ix = (long long)floorf(__fdiv_rn(__fsub_rn(xyz[3 * (size_t)i + 0], ci.org[0]), dl));
  const long long iy = (long long)floorf(__fdiv_rn(__fsub_rn(xyz[3 * (size_t)i + 1], ci.org[1]), dl));
  const long long iz = (long long)floorf(__fdiv_rn(__fsub_rn(xyz[3 * (size_t)i + 2], ci.org[2]), dl));
  const unsigned long long key = (unsigned long long)ix + (unsigned long long)ci.nx * (unsigned long long)iy +
                                 (unsigned long long)ci.nx * ci.ny * (unsigned long long)iz;
  // Sort field = the key's low 40 bits.  Unwrapped keys are < 2^40 or an error, as before.  A wrapped key w (as a
  // signed number in [-(1 + nx + nx ny), -1]) sorts as 2^40 + w: behind every unwrapped key of its cloud, which is
  // where the 64-bit order puts it, and distinct from all of them as long as the grid's nx ny nz cells end below it.
  unsigned long long flag = 0;
  if ((long long)key < 0) {
    flag = kKeyWrapped;
    const double cells = (double)ci.nx * (double)ci.ny * (double)ci.nz;
    if ((long long)key < -(1ll << (kKeyBits - 1)) || cells > (double)((1ll << kKeyBits) + (long long)key))
      atomicOr(err, 1);
  } else if (key > kKeyMask) {
    atomicOr(err, 1);
  }
  keys[i] = flag | ((unsigned long long)c << kKeyBits) | (key & kKeyMask);
  vals[i] = i;
}

__global__ void k_flags(const unsigned long long* __restrict__ keys, int n, int* flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// vid = exclusive scan of flags.  Writes voxel start offsets and nvox.
__global__ void k_segstart(const int* __restrict__ flags, const int* __restrict__ vid,
                           int n, int* vstart, int* nvox) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) vstart[vid[i]] = i;
  if (i == n - 1) *nvox = vid[i] + flags[i];
}

__global__ void k_bary(const float* __restrict__ xyz,
                       const unsigned long long* __restrict__ keys,
                       const int* __restrict__ vals, const int* __restrict__ vstart,
                       const int* __restrict__ nvox_p, int n, float* bary,
                       unsigned long long* vkey, int* vfirst) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int nvox = *nvox_p;
  if (v >= nvox) return;
  const int beg = vstart[v];
  const int end = (v + 1 < nvox) ? vstart[v + 1] : n;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int j = beg; j < end; ++j) {  // ascending original index (stable sort)
    const size_t p = (size_t)vals[j];
    sx = __fadd_rn(sx, xyz[3 * p + 0]);
    sy = __fadd_rn(sy, xyz[3 * p + 1]);
    sz = __fadd_rn(sz, xyz[3 * p + 2]);
  }
  // grid_subsampling.cpp:87: point * (1.0 / count)  -> float(double division)
  const float a = (float)(1.0 / (double)(end - beg));
  bary[3 * (size_t)v + 0] = __fmul_rn(sx, a);
  bary[3 * (size_t)v + 1] = __fmul_rn(sy, a);
  bary[3 * (size_t)v + 2] = __fmul_rn(sz, a);
  const unsigned long long k = keys[beg];
  vkey[v] = k;
  vfirst[v] = vals[beg];
}

// vcu[c] = first voxel of cloud c (voxels are sorted by (cloud, key)); one
// thread per cloud boundary, binary search instead of contended atomics.
__global__ void k_cloud_lb(const unsigned long long* __restrict__ vkey,
                           const int* __restrict__ nvox_p, int nb, int* vcu) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > nb) return;
  const int nvox = *nvox_p;
  int lo = 0, hi = nvox;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int)((vkey[mid] & ~kKeyWrapped) >> kKeyBits) < c)
      lo = mid + 1;
    else
      hi = mid;
  }
  vcu[c] = lo;
}

// Single workgroup: per-cloud voxel offsets (vcu), output lens / offsets.
__global__ void k_cloud_offsets(const int* __restrict__ vcu, int nb, int max_p, int* out_cu,
                                int* out_lens, int* out_total) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int b = 0;
  for (int c = 0; c < nb; ++c) {
    out_cu[c] = b;
    const int m = vcu[c + 1] - vcu[c];
    const int keep = (max_p > 0 && m > max_p) ? max_p : m;
    out_lens[c] = keep;
    b += keep;
  }
  out_cu[nb] = b;
  *out_total = b;
}

__global__ void k_emit_canonical(const float* __restrict__ bary,
                                 const unsigned long long* __restrict__ vkey,
                                 const int* __restrict__ nvox_p,
                                 const int* __restrict__ vcu,
                                 const int* __restrict__ out_cu,
                                 const int* __restrict__ out_lens, float* out, int* __restrict__ rowvox) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= *nvox_p) return;
  const int c = (int)((vkey[v] & ~kKeyWrapped) >> kKeyBits);
  const int r = v - vcu[c];
  if (r >= out_lens[c]) return;
  const size_t o = (size_t)(out_cu[c] + r);
  if (rowvox) rowvox[o] = v;   // output row -> voxel, for the attribute passes (NULL: plain call)
  out[3 * o + 0] = bary[3 * (size_t)v + 0];
  out[3 * o + 1] = bary[3 * (size_t)v + 1];
  out[3 * o + 2] = bary[3 * (size_t)v + 2];
}

// Insertion sequence of the voxels = ascending (cloud, first point index) = ascending first point
// index (clouds are contiguous): every voxel marks its first point, a scan over the points ranks the
// marks, a compaction emits the voxel ids in that order.  (A 64-bit pair sort did this before: 17
// merge-sort launches per subsampling.)
__global__ void k_mark_first(const int* __restrict__ vfirst, const int* __restrict__ nvox_p, int* __restrict__ mark,
                             int* __restrict__ who) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= *nvox_p) return;
  const int f = vfirst[v];
  mark[f] = 1;
  who[f] = v;
}
__global__ void k_compact_first(const int* __restrict__ mark, const int* __restrict__ pos, const int* __restrict__ who,
                                int n, int* __restrict__ ins) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !mark[i]) return;
  ins[pos[i]] = who[i];
}

// ---------------------------------------------------------------------------
// libstdc++ unordered_map iteration order, replayed per cloud.
//
// State after every rehash epoch is the node list L.  Within an epoch with
// `nbk` buckets the arrival sequence is  A = L_prev ++ (keys inserted in the
// epoch, in insertion order); the resulting list is: buckets in DESCENDING
// order of the arrival position of their first node, each bucket's nodes in
// DESCENDING arrival position (hashtable.h _M_insert_bucket_begin /
// _M_rehash_aux: a node goes to the list head if its bucket is empty, else to
// the head of its bucket's chain).  Verified against std::unordered_map in
// tests/test_oracle_native.py (oracle) and tests/test_preprocess_gpu.py.
//
// Per epoch, in parallel over arrival positions p:
//   first[b] = min p, cnt[b]++, chain push          (atomics)
//   P = inclusive scan of (p is bucket head ? cnt[b] : 0)
//   new position = (total - P[first[b]]) + #{same bucket, pos > p}
// One 1024-thread workgroup per cloud; tables live in the global workspace.
__device__ void block_inclusive_scan(int* data, int m, int* lds /*[1024]*/) {
  const int t = threadIdx.x, T = blockDim.x;
  const int per = (m + T - 1) / T;
  const int beg = min(t * per, m), end = min(beg + per, m);
  int s = 0;
  for (int i = beg; i < end; ++i) s += data[i];
  lds[t] = s;
  __syncthreads();
  for (int o = 1; o < T; o <<= 1) {
    int v = (t >= o) ? lds[t - o] : 0;
    __syncthreads();
    lds[t] += v;
    __syncthreads();
  }
  int run = lds[t] - s;
  for (int i = beg; i < end; ++i) {
    run += data[i];
    data[i] = run;
  }
  __syncthreads();
}

// k % nbk for k < 2^40 (voxel keys), nbk < 2^32: quotient estimate in double (off by at most one), exact fix-up.
__device__ __forceinline__ int fast_mod(unsigned long long k, unsigned int nbk, double inv) {
  const unsigned long long q = (unsigned long long)((double)k * inv);
  long long r = (long long)k - (long long)(q * (unsigned long long)nbk);
  if (r < 0) r += nbk;
  else if (r >= (long long)nbk) r -= nbk;
  return (int)r;
}

// bucket tables (first arrival, count, chain head) of an epoch live in LDS while 3 * nbk ints fit
constexpr int kUmapLdsInts = 31744;   // 124 KB: every epoch up to 10 273 buckets (clouds of <= 10 273 voxels)

__global__ __launch_bounds__(1024) void k_umap_order(
    const unsigned long long* __restrict__ vkey, const int* __restrict__ ins,
    const int* __restrict__ vcu, const int* __restrict__ cu, int nsched, SchedArg sched,
    int* listA, int* listB, int* tfirst, int* tcnt, int* thead, int* nxt,
    int* scan, int* bucket, const float* __restrict__ bary, const int* __restrict__ out_cu,
    const int* __restrict__ out_lens, float* out, int* __restrict__ rowvox) {
  __shared__ int lds[1024];
  extern __shared__ int lds_tab[];
  const int c = blockIdx.x;
  const int base = vcu[c];
  const int m = vcu[c + 1] - base;
  if (m <= 0) return;
  // per-cloud slices of the workspace
  int* la = listA + base;
  int* lb = listB + base;
  int* nx = nxt + base;
  int* sc = scan + base;
  int* bk = bucket + base;
  const size_t toff = 3 * (size_t)cu[c] + 16 * (size_t)c;
  const int t = threadIdx.x, T = blockDim.x;

  int done = 0;  // elements already in the list
  int e = 0;
  int* cur = la;
  int* nxtl = lb;
  while (done < m) {
    e += 1;
    if (e >= nsched) break;  // cannot happen: schedule covers 4M voxels
    const int nbk = (int)sched.v[e];
    const int upto = min(m, nbk);
    const int len = upto;  // arrival sequence length = done + (upto - done)
    const double inv = 1.0 / (double)nbk;
    auto epoch = [&](int* tf, int* tc, int* th) {
      for (int b = t; b < nbk; b += T) {
        tf[b] = 0x7fffffff;
        tc[b] = 0;
        th[b] = -1;
      }
      // new arrivals are elements done..upto-1 (insertion order)
      for (int p = done + t; p < upto; p += T) cur[p] = p;
      __syncthreads();
      for (int p = t; p < len; p += T) {
        const int el = cur[p];
        const unsigned long long vk = vkey[ins[base + el]];
        // a wrapped key hashes with all its 64 bits (identity hash of the reference's size_t key): plain modulo, rare
        const int b = (vk & kKeyWrapped) ? (int)((vk | ~kKeyMask) % (unsigned long long)nbk)
                                         : fast_mod(vk & kKeyMask, (unsigned int)nbk, inv);
        bk[p] = b;
        atomicMin(&tf[b], p);
        atomicAdd(&tc[b], 1);
        nx[p] = atomicExch(&th[b], p);
      }
      __syncthreads();
      for (int p = t; p < len; p += T) {
        const int b = bk[p];
        sc[p] = (tf[b] == p) ? tc[b] : 0;
      }
      __syncthreads();
      block_inclusive_scan(sc, len, lds);
      const int total = len;  // sum of all bucket counts
      for (int p = t; p < len; p += T) {
        const int b = bk[p];
        int greater = 0;
        for (int q = th[b]; q != -1; q = nx[q]) greater += (q > p) ? 1 : 0;
        const int pos = (total - sc[tf[b]]) + greater;
        nxtl[pos] = cur[p];
      }
      __syncthreads();
    };
    if (3 * nbk <= kUmapLdsInts) epoch(lds_tab, lds_tab + nbk, lds_tab + 2 * nbk);
    else epoch(tfirst + toff, tcnt + toff, thead + toff);
    int* tmp = cur;
    cur = nxtl;
    nxtl = tmp;
    done = upto;
  }
  // emit in list order
  const int keep = out_lens[c];
  const size_t ob = (size_t)out_cu[c];
  for (int p = t; p < keep; p += T) {
    const size_t v = (size_t)ins[base + cur[p]];
    out[3 * (ob + p) + 0] = bary[3 * v + 0];
    out[3 * (ob + p) + 1] = bary[3 * v + 1];
    out[3 * (ob + p) + 2] = bary[3 * v + 2];
    if (rowvox) rowvox[ob + p] = (int)v;
  }
}

__global__ void k_check_err(const int* err, int* out_total) {
  if (*err) *out_total = -1;
}

size_t sort_temp_bytes(int n) {
  size_t bytes = 0;
  rocprim::radix_sort_pairs(nullptr, bytes, (unsigned long long*)nullptr,
                            (unsigned long long*)nullptr, (int*)nullptr, (int*)nullptr,
                            (unsigned int)(n > 0 ? n : 1));
  size_t sb = 0;
  rocprim::exclusive_scan(nullptr, sb, (int*)nullptr, (int*)nullptr, 0, (size_t)(n > 0 ? n : 1),
                          rocprim::plus<int>());
  return align_up(bytes > sb ? bytes : sb, 256) + 256;
}

// Sizes (n, nb) below 1 are measured as 1 (the size query's clamp).
struct SubsampleWs {
  CloudInfo* info;
  unsigned long long *keys, *keys2, *vkey;
  int *vals, *vals2, *flags, *vid, *vstart, *vfirst, *sval, *sval2, *listA, *listB, *nxt, *scan;
  float* bary;
  int *tfirst, *tcnt, *thead;   // bucket tables
  int *cloud_cnt, *vcu, *out_cu;
  int* scalars;                 // [0]=nvox [1]=err
  size_t temp_bytes;
  void* temp;
};
SubsampleWs subsample_layout(Workspace& w, int n, int nb) {
  const size_t N = (size_t)(n > 0 ? n : 1), B = (size_t)(nb > 0 ? nb : 1);
  SubsampleWs l;
  l.info = w.take<CloudInfo>(B);
  l.keys = w.take<unsigned long long>(N);
  l.keys2 = w.take<unsigned long long>(N);
  l.vkey = w.take<unsigned long long>(N);
  for (int** p : {&l.vals, &l.vals2, &l.flags, &l.vid, &l.vstart, &l.vfirst, &l.sval, &l.sval2, &l.listA, &l.listB, &l.nxt,
                  &l.scan})
    *p = w.take<int>(N);
  l.bary = w.take<float>(3 * N);
  const size_t tsz = 3 * N + 16 * B + 64;
  l.tfirst = w.take<int>(tsz);
  l.tcnt = w.take<int>(tsz);
  l.thead = w.take<int>(tsz);
  l.cloud_cnt = w.take<int>(B + 1);
  l.vcu = w.take<int>(B + 1);
  l.out_cu = w.take<int>(B + 1);
  l.scalars = w.take<int>(64);
  l.temp_bytes = sort_temp_bytes(n);
  l.temp = w.take<char>(l.temp_bytes);
  // unused (a fourth per-cloud array and 768 scalar bytes that the size query has always counted): no kernel is handed
  // a pointer into them; kept so that the size callers see does not change
  (void)w.take<int>(B + 1);
  (void)w.take<char>(768);
  return l;
}

SchedArg sched_arg(const Schedule& s, int* nsched) {
  SchedArg sched;
  for (int i = 0; i < kMaxSched; ++i)
    sched.v[i] = i < (int)s.buckets.size() ? s.buckets[i] : 0xffffffffu;
  *nsched = (int)(s.buckets.size() < (size_t)kMaxSched ? s.buckets.size() : kMaxSched);
  return sched;
}

// Everything both entry points enqueue, up to the emitted points; the caller ends with k_check_err.  Left behind for
// the attribute passes: vals2 (point indices sorted by voxel, original order inside a voxel), scalars[0] (voxel
// count), out_cu, and -- only when the caller hands in `rank` and `rowvox` -- vstart (segment starts) and rowvox
// (output row -> voxel, after the order mode and the max_p cut).  The plain call passes NULL for both: the insertion
// ranks then overwrite vstart, as they always have.
int subsample_enqueue(const SubsampleWs& l, const float* xyz, const int* cu, int n, int nb, float dl, int max_p,
                      int order_mode, float* out_xyz, int* out_lens, int* out_total, int* rank, int* rowvox,
                      hipStream_t stream) {
  const auto [info, keys, keys2, vkey, vals, vals2, flags, vid, vstart, vfirst, sval, sval2, listA, listB, nxt, scan, bary,
              tfirst, tcnt, thead, cloud_cnt, vcu, out_cu, scalars, temp_bytes, temp] = l;
  if (!rank) rank = vstart;
  const size_t N = (size_t)n;
  int* nvox = scalars;
  int* err = scalars + 1;

  SPR_HIP_CHECK(hipMemsetAsync(scalars, 0, 64 * sizeof(int), stream));
  SPR_HIP_CHECK(hipMemsetAsync(cloud_cnt, 0, (nb + 1) * sizeof(int), stream));

  const int TB = 256;
  hipLaunchKernelGGL(k_bbox, dim3(nb), dim3(256), 0, stream, xyz, cu, dl, info);
  hipLaunchKernelGGL(k_keys, dim3(cdiv(n, TB)), dim3(TB), 0, stream, xyz, cu, n, nb, dl,
                     info, keys, vals, err);
  SPR_LAUNCH_CHECK();
  size_t tb = temp_bytes;
  // keys = cloud << kKeyBits | voxel: only the bits a batch of nb clouds can set are sorted (6 radix passes instead
  // of 8 for 128 clouds)
  int key_bits = kKeyBits + 1;
  while (key_bits < 64 && (1ull << (key_bits - kKeyBits)) < (unsigned long long)nb) ++key_bits;
  SPR_HIP_CHECK(rocprim::radix_sort_pairs(temp, tb, keys, keys2, vals, vals2,
                                          (unsigned int)n, 0, key_bits, stream));
  hipLaunchKernelGGL(k_flags, dim3(cdiv(n, TB)), dim3(TB), 0, stream, keys2, n, flags);
  tb = temp_bytes;
  SPR_HIP_CHECK(rocprim::exclusive_scan(temp, tb, flags, vid, 0, (size_t)n,
                                        rocprim::plus<int>(), stream));
  hipLaunchKernelGGL(k_segstart, dim3(cdiv(n, TB)), dim3(TB), 0, stream, flags, vid, n,
                     vstart, nvox);
  hipLaunchKernelGGL(k_bary, dim3(cdiv(n, TB)), dim3(TB), 0, stream, xyz, keys2, vals2,
                     vstart, nvox, n, bary, vkey, vfirst);
  hipLaunchKernelGGL(k_cloud_lb, dim3(cdiv(nb + 1, 256)), dim3(256), 0, stream, vkey, nvox, nb, vcu);
  hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(64), 0, stream, vcu, nb, max_p, out_cu,
                     out_lens, out_total);
  SPR_LAUNCH_CHECK();
  if (order_mode == SPR_ORDER_CANONICAL) {
    hipLaunchKernelGGL(k_emit_canonical, dim3(cdiv(n, TB)), dim3(TB), 0, stream, bary,
                       vkey, nvox, vcu, out_cu, out_lens, out_xyz, rowvox);
  } else {
    int nsched;
    const SchedArg sched = sched_arg(host_schedule(), &nsched);
    // insertion order: flags / vid / vstart are free again after k_bary (mark, who, rank)
    SPR_HIP_CHECK(hipMemsetAsync(flags, 0, N * sizeof(int), stream));
    hipLaunchKernelGGL(k_mark_first, dim3(cdiv(n, TB)), dim3(TB), 0, stream, vfirst, nvox, flags, vid);
    tb = temp_bytes;
    SPR_HIP_CHECK(rocprim::exclusive_scan(temp, tb, flags, rank, 0, (size_t)n, rocprim::plus<int>(), stream));
    hipLaunchKernelGGL(k_compact_first, dim3(cdiv(n, TB)), dim3(TB), 0, stream, flags, rank, vid, n, sval2);
    const int umap_lds = kUmapLdsInts * (int)sizeof(int);
    if (int rc = ensure_dyn_lds((const void*)k_umap_order, umap_lds)) return rc;
    hipLaunchKernelGGL(k_umap_order, dim3(nb), dim3(1024), umap_lds, stream, vkey, sval2, vcu, cu,
                       nsched, sched, listA, listB, tfirst, tcnt, thead, nxt, scan, sval, bary, out_cu,
                       out_lens, out_xyz, rowvox);
  }
  SPR_LAUNCH_CHECK();
  return 0;
}

// ---- attributes: feature average and label vote per voxel -------------------------------------------------------------
// One thread per (output row, column), the column fastest: the threads of a row read one point's attribute row together.
// Each walks its voxel's segment of vals2 in order, which is the original point order (stable sort), as k_bary does.
struct Segment {
  int beg, end;
};
__device__ __forceinline__ Segment segment_of(int v, const int* __restrict__ vstart, int nvox, int n) {
  return {vstart[v], (v + 1 < nvox) ? vstart[v + 1] : n};
}

// grid_subsampling.h:46,59 (float32 sum in point order, from +0) and grid_subsampling.cpp:90-94 (one division by
// (float)count -- not the barycentre's multiplication by a reciprocal).
__global__ void k_attr_features(const float* __restrict__ feat, int fdim, const int* __restrict__ vals,
                                const int* __restrict__ vstart, const int* __restrict__ nvox_p, int n,
                                const int* __restrict__ rowvox, const int* __restrict__ out_cu, int nb,
                                float* __restrict__ out_feat) {
  const size_t total = (size_t)out_cu[nb] * (size_t)fdim;
  const int nvox = *nvox_p;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const size_t row = t / (size_t)fdim;
    const size_t col = t - row * (size_t)fdim;
    const Segment s = segment_of(rowvox[row], vstart, nvox, n);
    float sum = 0.f;
    for (int j = s.beg; j < s.end; ++j) sum = __fadd_rn(sum, feat[(size_t)vals[j] * (size_t)fdim + col]);
    out_feat[t] = __fdiv_rn(sum, (float)(s.end - s.beg));
  }
}

// std::hash<int> is the value converted to size_t, i.e. sign extended; the bucket is hash % bucket_count.
__device__ __forceinline__ int label_bucket(int label, unsigned int nbk) {
  return (int)((unsigned long long)(long long)label % (unsigned long long)nbk);
}
// One insertion into the node list of a libstdc++ hashtable (hashtable.h _M_insert_bucket_begin, and _M_rehash_aux,
// which re-inserts by the same rule): the node goes to the list's front if its bucket is empty, else directly in front
// of the first node of its bucket.  list: key numbers (first-arrival rank), bkt: bucket per key number.
__device__ __forceinline__ int list_insert(int* __restrict__ list, int len, int id, const int* __restrict__ bkt) {
  const int b = bkt[id];
  int at = 0;
  while (at < len && bkt[list[at]] != b) ++at;
  if (at == len) at = 0;
  for (int j = len; j > at; --j) list[j] = list[j - 1];
  list[at] = id;
  return len + 1;
}

// grid_subsampling.h:50,69 (labels[i][*it] += 1 in point order) and grid_subsampling.cpp:99-101 (max_element over the
// map's iteration order with `<` on the counts: the first maximum in that order wins).
// The thread keeps its voxel's distinct labels and their counts in first-arrival order in its segment's slice of
// dist / cnt (a segment of k points has at most k distinct labels); only a tied maximum needs the iteration order,
// and then the container's node list is replayed in the same slice of la / lb / bkt: epoch e of the bucket schedule
// re-inserts the list front to back under sched[e] buckets and appends the keys that arrive before the next growth
// (the k-th distinct key, k counted from 0, arrives when the table has sched[e] > k buckets: k_umap_order's epochs).
__global__ void k_attr_labels(const int* __restrict__ lab, int ldim, const int* __restrict__ vals,
                              const int* __restrict__ vstart, const int* __restrict__ nvox_p, int n,
                              const int* __restrict__ rowvox, const int* __restrict__ out_cu, int nb, int nsched,
                              SchedArg sched, int* __restrict__ dist, int* __restrict__ cnt, int* __restrict__ la,
                              int* __restrict__ lb, int* __restrict__ bkt, int* __restrict__ out_lab, int* err) {
  const size_t total = (size_t)out_cu[nb] * (size_t)ldim;
  const int nvox = *nvox_p;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const size_t row = t / (size_t)ldim;
    const size_t col = t - row * (size_t)ldim;
    const Segment s = segment_of(rowvox[row], vstart, nvox, n);
    const size_t slice = col * (size_t)n + (size_t)s.beg;
    int* d = dist + slice;
    int* c = cnt + slice;
    int m = 0;
    for (int j = s.beg; j < s.end; ++j) {
      const int l = lab[(size_t)vals[j] * (size_t)ldim + col];
      int k = 0;
      while (k < m && d[k] != l) ++k;
      if (k == m) {
        d[m] = l;
        c[m] = 1;
        ++m;
      } else {
        c[k] += 1;
      }
    }
    int best = 0, tied = 1;
    for (int k = 1; k < m; ++k) {
      if (c[k] > c[best]) {
        best = k;
        tied = 1;
      } else if (c[k] == c[best]) {
        ++tied;
      }
    }
    if (tied > 1) {
      const int top = c[best];
      int* cur = la + slice;
      int* other = lb + slice;
      int* bk = bkt + slice;
      int len = 0, done = 0, e = 0;
      while (done < m) {
        e += 1;
        if (e >= nsched) {   // cannot happen: the host measured the schedule for n keys
          atomicOr(err, 1);
          break;
        }
        const unsigned int nbk = sched.v[e];
        const int upto = (unsigned int)m < nbk ? m : (int)nbk;
        for (int k = 0; k < upto; ++k) bk[k] = label_bucket(d[k], nbk);
        int relen = 0;
        for (int i = 0; i < len; ++i) relen = list_insert(other, relen, cur[i], bk);
        int* tmp = cur;
        cur = other;
        other = tmp;
        for (int k = done; k < upto; ++k) len = list_insert(cur, len, k, bk);
        done = upto;
      }
      for (int i = 0; i < len; ++i) {
        if (c[cur[i]] == top) {
          best = cur[i];
          break;
        }
      }
    }
    out_lab[t] = d[best];
  }
}

// The plain layout, then what the attribute passes add: rank (the insertion ranks, so that vstart survives), rowvox,
// and five ints per (point, label column) for the vote.  Nothing depends on fdim.
struct AttrsWs {
  SubsampleWs sub;
  int *rank, *rowvox, *dist, *cnt, *la, *lb, *bkt;
};
AttrsWs attrs_layout(Workspace& w, int n, int nb, int fdim, int ldim) {
  const size_t N = (size_t)(n > 0 ? n : 1), L = (size_t)(ldim > 0 ? ldim : 0);
  (void)fdim;
  AttrsWs l;
  l.sub = subsample_layout(w, n, nb);
  l.rank = w.take<int>(N);
  l.rowvox = w.take<int>(N);
  for (int** p : {&l.dist, &l.cnt, &l.la, &l.lb, &l.bkt}) *p = w.take<int>(N * L);
  return l;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_grid_subsample_workspace_bytes(int n, int nb) {
  return measure(subsample_layout, n, nb);
}

extern "C" int spr_grid_subsample(const float* xyz, const int* cu, int n, int nb,
                                  float dl, int max_p, int order_mode,
                                  float* out_xyz, int* out_lens, int* out_total,
                                  void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(n >= 0 && nb >= 1, "grid_subsample: bad sizes n=%d nb=%d", n, nb);
  SPR_REQUIRE(dl > 0.f, "grid_subsample: sampleDl must be > 0");
  SPR_REQUIRE(nb < (1 << 23), "grid_subsample: too many clouds");
  // reference: subsampling an empty batch is an error (wrapper.cpp:266-270)
  SPR_REQUIRE(n > 0, "grid_subsample: empty input");
  Workspace w(ws, ws_bytes);
  const SubsampleWs l = subsample_layout(w, n, nb);
  SPR_REQUIRE(ws != nullptr && w.ok(), "grid_subsample: workspace too small");
  if (int rc = subsample_enqueue(l, xyz, cu, n, nb, dl, max_p, order_mode, out_xyz, out_lens, out_total, nullptr, nullptr,
                                 stream))
    return rc;
  hipLaunchKernelGGL(k_check_err, dim3(1), dim3(1), 0, stream, l.scalars + 1, out_total);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spr_grid_subsample_attrs_workspace_size(int n, int nb, int fdim, int ldim) {
  return measure(attrs_layout, n, nb, fdim, ldim);
}

extern "C" int spr_grid_subsample_attrs(const float* xyz, const int* cu, int n, int nb, float dl, int max_p,
                                        int order_mode, const float* feat, int fdim, const int* lab, int ldim,
                                        float* out_xyz, float* out_feat, int* out_lab, int* out_lens, int* out_total,
                                        void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(n >= 0 && nb >= 1, "grid_subsample_attrs: bad sizes n=%d nb=%d", n, nb);
  SPR_REQUIRE(dl > 0.f, "grid_subsample_attrs: sampleDl must be > 0");
  SPR_REQUIRE(nb < (1 << 23), "grid_subsample_attrs: too many clouds");
  SPR_REQUIRE(n > 0, "grid_subsample_attrs: empty input");
  SPR_REQUIRE(fdim >= 0 && ldim >= 0, "grid_subsample_attrs: negative dimension fdim=%d ldim=%d", fdim, ldim);
  SPR_REQUIRE(fdim == 0 || (feat && out_feat), "grid_subsample_attrs: fdim=%d without features in and out", fdim);
  SPR_REQUIRE(ldim == 0 || (lab && out_lab), "grid_subsample_attrs: ldim=%d without labels in and out", ldim);
  Workspace w(ws, ws_bytes);
  const AttrsWs l = attrs_layout(w, n, nb, fdim, ldim);
  SPR_REQUIRE(ws != nullptr && w.ok(), "grid_subsample_attrs: workspace too small");
  int nsched = 0;
  SchedArg sched;
  if (ldim > 0) sched = sched_arg(label_schedule((size_t)n), &nsched);   // host work: before anything is enqueued
  if (int rc = subsample_enqueue(l.sub, xyz, cu, n, nb, dl, max_p, order_mode, out_xyz, out_lens, out_total, l.rank,
                                 l.rowvox, stream))
    return rc;
  const int TB = 256;
  const long kMaxBlocks = 1 << 20;   // grid-stride beyond: n * dim has no int bound
  int* nvox = l.sub.scalars;
  if (fdim > 0) {
    const long blocks = ((long)n * fdim + TB - 1) / TB;
    hipLaunchKernelGGL(k_attr_features, dim3((unsigned int)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), dim3(TB), 0,
                       stream, feat, fdim, l.sub.vals2, l.sub.vstart, nvox, n, l.rowvox, l.sub.out_cu, nb, out_feat);
  }
  if (ldim > 0) {
    const long blocks = ((long)n * ldim + TB - 1) / TB;
    hipLaunchKernelGGL(k_attr_labels, dim3((unsigned int)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), dim3(TB), 0,
                       stream, lab, ldim, l.sub.vals2, l.sub.vstart, nvox, n, l.rowvox, l.sub.out_cu, nb, nsched, sched,
                       l.dist, l.cnt, l.la, l.lb, l.bkt, out_lab, l.sub.scalars + 1);
  }
  hipLaunchKernelGGL(k_check_err, dim3(1), dim3(1), 0, stream, l.sub.scalars + 1, out_total);
  SPR_LAUNCH_CHECK();
  return 0;
}

// ---- spatial walk order -----------------------------------------------------------------------------
// order[] = the points of every cloud sorted by the Morton code of their `cell`-sized grid cell (clouds in batch
// order).  Not part of any result: operators that gather rows of the PREVIOUS level for every point (max-pool, the
// first convolution) walk their queries in this order so that queries in flight together share neighbours and the
// rows they gather are served by L2 instead of being re-fetched from HBM (the points themselves stay in the
// reference's hash-map order).  The grid origin of a cloud is its first point: any fixed origin does.
namespace spr {
namespace {
__device__ __forceinline__ unsigned int spread10(unsigned int v) {     // 10 bits -> every third bit
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__global__ void k_order_keys(const float* __restrict__ xyz, const int* __restrict__ cu, int n, int nb, float inv_cell,
                             unsigned long long* __restrict__ keys, int* __restrict__ vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = nb;                               // cloud of point i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= i) lo = mid; else hi = mid;
  }
  const int o = cu[lo];
  unsigned int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float d = (xyz[3 * (size_t)i + a] - xyz[3 * (size_t)o + a]) * inv_cell;
    const int q = (int)floorf(fminf(fmaxf(d, -512.f), 511.f)) + 512;
    c[a] = (unsigned int)q;
  }
  const unsigned int m = spread10(c[0]) | (spread10(c[1]) << 1) | (spread10(c[2]) << 2);
  keys[i] = ((unsigned long long)lo << 30) | m;
  vals[i] = i;
}
}  // namespace
}  // namespace spr

namespace spr {
namespace {
struct CellOrderWs {
  unsigned long long *keys, *keys2;
  int* vals;
  size_t temp_bytes;
  void* temp;
};
CellOrderWs cell_order_layout(Workspace& w, int n) {
  const size_t N = (size_t)(n > 0 ? n : 1);
  CellOrderWs l;
  l.keys = w.take<unsigned long long>(N);
  l.keys2 = w.take<unsigned long long>(N);
  l.vals = w.take<int>(N);
  l.temp_bytes = sort_temp_bytes(n);
  l.temp = w.take<char>(l.temp_bytes);
  (void)w.take<char>(256);   // unused: the size query has always counted it, and callers see the same size as before
  return l;
}
}  // namespace
}  // namespace spr

extern "C" size_t spr_cell_order_workspace_bytes(int n) {
  return measure(cell_order_layout, n);
}

extern "C" int spr_cell_order(const float* xyz, const int* cu, int n, int nb, float cell, int* order, void* ws,
                              size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(n >= 1 && nb >= 1 && nb < (1 << 30) && cell > 0.f, "cell_order: bad arguments");
  Workspace w(ws, ws_bytes);
  auto [keys, keys2, vals, tb, temp] = cell_order_layout(w, n);
  SPR_REQUIRE(ws != nullptr && w.ok(), "cell_order: workspace too small");
  hipLaunchKernelGGL(k_order_keys, dim3(cdiv(n, 256)), dim3(256), 0, stream, xyz, cu, n, nb, 1.0f / cell, keys, vals);
  SPR_LAUNCH_CHECK();
  int bits = 31;
  while (bits < 60 && (1ull << (bits - 30)) < (unsigned long long)nb) ++bits;
  SPR_HIP_CHECK(rocprim::radix_sort_pairs(temp, tb, keys, keys2, vals, order, (unsigned int)n, 0, bits, stream));
  return 0;
}

// ---- voxel pre-downsampling, one point per voxel -----------------------------------
// Replaces the CPU voxel_down_sample of the KITTI loader (data_loaders/kitti_pred.py:12-14, :203-204,
// kiss_icp: voxel = (p / voxel_size) truncated toward zero per axis; the FIRST point that falls
// into a voxel is kept).  The kept SET of points is the reference's; they are emitted in
// ascending original index (kiss_icp emits hash-map order, which nothing downstream depends on).
namespace spr {
namespace {
__global__ void k_vox_keys(const float* __restrict__ xyz, int n, double voxel, unsigned long long* keys,
                           int* vals, int* err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long k = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double q = (double)xyz[3 * (size_t)i + d] / voxel;   // Eigen: (point / voxel_size).cast<int>()
    const long long c = (long long)q;                                    // truncation toward zero
    if (c < -(1ll << 20) || c >= (1ll << 20)) atomicExch(err, 1);
    k = (k << 21) | (unsigned long long)((c + (1ll << 20)) & 0x1fffff);
  }
  keys[i] = k;
  vals[i] = i;
}
__global__ void k_vox_heads(const unsigned long long* __restrict__ keys, const int* __restrict__ vals, int n,
                            unsigned int* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // stable sort: the first entry of an equal-key run carries the smallest original index
  const bool head = i == 0 || keys[i] != keys[i - 1];
  out[i] = head ? (unsigned int)vals[i] : 0xffffffffu;
}
__global__ void k_vox_count(const unsigned int* __restrict__ sorted, int n, int* out_idx, int* count,
                            const int* err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool ok = sorted[i] != 0xffffffffu;
  out_idx[i] = ok ? (int)sorted[i] : -1;
  if (ok && (i + 1 == n || sorted[i + 1] == 0xffffffffu)) count[0] = err[0] ? -1 : i + 1;
}
size_t vox_temp_bytes(int n) {
  size_t a = 0, b = 0;
  rocprim::radix_sort_pairs(nullptr, a, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int*)nullptr,
                            (int*)nullptr, (unsigned int)(n > 0 ? n : 1), 0, 63);
  rocprim::radix_sort_keys(nullptr, b, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int)(n > 0 ? n : 1), 0,
                           32);
  return align_up(a > b ? a : b, 256);
}
struct VoxelWs {
  unsigned long long *keys, *keys2;
  int *vals, *vals2;
  unsigned int *sel, *sel2;
  int* err;
  size_t temp_bytes;
  void* temp;
};
VoxelWs voxel_layout(Workspace& w, int n) {
  const size_t N = (size_t)(n > 0 ? n : 1);
  VoxelWs l;
  l.keys = w.take<unsigned long long>(N);
  l.keys2 = w.take<unsigned long long>(N);
  l.vals = w.take<int>(N);
  l.vals2 = w.take<int>(N);
  l.sel = w.take<unsigned int>(N);
  l.sel2 = w.take<unsigned int>(N);
  l.err = w.take<int>(1);
  l.temp_bytes = vox_temp_bytes(n);
  l.temp = w.take<char>(l.temp_bytes);
  return l;
}
}  // namespace
}  // namespace spr

extern "C" size_t spr_voxel_downsample_workspace_bytes(int n) {
  return measure(spr::voxel_layout, n);
}

// out_idx [n] i32: the first out_count[0] entries are the kept original indices (ascending);
// out_count[0] = -1 if a coordinate exceeds +-2^20 voxels.
extern "C" int spr_voxel_downsample(const float* xyz, int n, double voxel_size, int* out_idx, int* out_count, void* ws,
                                    size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(n >= 1 && voxel_size > 0.0 && xyz && out_idx && out_count, "voxel_downsample: bad arguments");
  Workspace w(ws, ws_bytes);
  const auto [keys, keys2, vals, vals2, sel, sel2, err, temp_bytes, temp] = voxel_layout(w, n);
  SPR_REQUIRE(ws != nullptr && w.ok(), "voxel_downsample: workspace too small");
  SPR_HIP_CHECK(hipMemsetAsync(err, 0, sizeof(int), stream));
  SPR_HIP_CHECK(hipMemsetAsync(out_count, 0, sizeof(int), stream));
  const int TBk = 256;
  hipLaunchKernelGGL(k_vox_keys, dim3(cdiv(n, TBk)), dim3(TBk), 0, stream, xyz, n, voxel_size, keys, vals, err);
  size_t tb = temp_bytes;
  SPR_HIP_CHECK(rocprim::radix_sort_pairs(temp, tb, keys, keys2, vals, vals2, (unsigned int)n, 0, 63, stream));
  hipLaunchKernelGGL(k_vox_heads, dim3(cdiv(n, TBk)), dim3(TBk), 0, stream, keys2, vals2, n, sel);
  tb = temp_bytes;
  SPR_HIP_CHECK(rocprim::radix_sort_keys(temp, tb, sel, sel2, (unsigned int)n, 0, 32, stream));
  hipLaunchKernelGGL(k_vox_count, dim3(cdiv(n, TBk)), dim3(TBk), 0, stream, sel2, n, out_idx, out_count, err);
  SPR_LAUNCH_CHECK();
  return 0;
}
